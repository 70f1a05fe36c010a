"""The session walks' CPU side (tests/session_walk.py): no GPU needed.

  a. the plans reach the states they are meant for -- asserted on the reference's trace alone
  b. the reference agrees with what it is built from: every utterance in which no horizon pruned ends with the
     labels and the score of oracle.decode (primed ones: primed_ref.primed_decode), bit for bit
  c. ... and, push by push and commit by commit, with commit_ref.ReplaySession over nbest_ref.replay: the oracle's
     own candidate scores, pruned again in numpy, and a second statement of the commit rule
"""

import numpy as np
import pytest

import commit_ref
import nbest_ref
import primed_ref
import session_walk as sw
from oracle import oracle

FULL = ('small4', 'small10', 'deep', 'embedded')   # the plans that must reach every state; one_launch is a short script
# where a beam that no horizon pruned agrees on two frames or more at some commit (a wide beam seldom does)
COMMITTING = ('small4', 'one_launch')
INF_BITS = int(np.array(np.inf, dtype=np.float32).view(np.uint32))


# ---- a. the plans reach their states

@pytest.mark.parametrize('name', FULL)
def test_the_plan_reaches_its_states(name, oracle_lib):
  tr = sw.walk(name)
  f = sw.facts(tr)
  case = sw.CASES[name]
  # every kind of operation at least three times (the three refused calls are one kind: each of them occurs once)
  assert all(f['kinds'][k] >= 3 for k in sw.KINDS), f['kinds']
  assert f['bad_frames'] >= 1
  # every pair of kinds that can follow each other on one slot
  assert f['pairs'] == set(sw.PAIRS), set(sw.PAIRS) - f['pairs']
  # commits: hypotheses dropped; retained rows that overlap their source and rows that do not; an empty window; an
  # emptied beam; a horizon larger than have (facts() asserts that it commits the stable prefix and drops nothing)
  assert all(f['commits'][k] >= 1 for k in ('dropped', 'overlap', 'no_overlap', 'have_0', 'empty_beam', 'far_horizon')), f['commits']
  # restarts: odd and even windows, an empty window behind a commit, a committed part, an emptied beam, a slot that
  # never received a frame, one slot twice
  assert all(f['restarts'][k] >= 1 for k in ('odd', 'even', 'emptied_window', 'committed', 'empty_beam', 'never')), f['restarts']
  assert f['restarts']['same_slot_twice']
  # primes: a just-restarted slot between an odd and an even neighbour; the whole window, and the next commit frees room
  assert f['primes']['restarted_between_odd_and_even'] >= 1 and f['primes']['whole_window_then_room'] >= 1, f['primes']
  # more than 2 * max_frames + 2 frames through one utterance, and through another slot across a restart: the prior
  # tables (max_frames + 2 entries at uis_stream_begin) have to grow
  assert f['one_life_outgrows_the_tables'] and f['a_slot_outgrows_the_tables_across_a_restart'] and f['tables_grew']
  assert f['a_pruned_beam_fills_up_again']
  assert f['a_push_fills_a_window']
  # each refused call once, in a session with committed frames and wide beams
  assert f['refusals'] == {'push': 1, 'prime_received': 1, 'prime_long': 1}, f['refusals']
  # the budgets: about 120 operations and 400 - 600 frames (small), about 60 operations (the others)
  if case['plan'] == 'small':
    assert 100 <= f['operations'] <= 130 and 400 <= f['frames'] <= 600, (f['operations'], f['frames'])
  else:
    assert 50 <= f['operations'] <= 70, f['operations']
  assert tr['max_clusters'] < case['cap']


def test_the_short_plan_of_the_one_launch_shape(oracle_lib):
  """At most 90 frames (the reference takes a sixth of a second per frame and utterance at this size): prime, push,
  commit with horizons, restart, prime again, push, commit, one refused call -- and the states those reach."""
  tr = sw.walk('one_launch')
  f = sw.facts(tr)
  assert f['frames'] <= 90, f['frames']
  assert [st['kind'] for st in tr['steps']][:6] == ['prime', 'push', 'push', 'commit_h', 'restart', 'prime']
  assert f['kinds']['refuse'] == 1 and f['refusals'] == {'push': 1}
  assert {('push', 'commit'), ('commit_h', 'restart'), ('restart', 'prime'), ('restart', 'push'), ('commit', 'push')} <= f['pairs']
  assert f['commits']['dropped'] >= 1 and f['commits']['overlap'] >= 1 and f['commits']['no_overlap'] >= 1
  assert f['restarts']['odd'] >= 1 and f['restarts']['even'] >= 1 and f['restarts']['committed'] >= 1
  assert f['primes']['restarted_between_odd_and_even'] >= 1
  assert f['a_pruned_beam_fills_up_again'] and f['tables_grew']
  # a push of at least four frames per slot: the default path of this shape takes it in one launch
  assert any(st['kind'] == 'push' and max(len(c) for c in st['call']['chunks'] if c is not None) >= 4 for st in tr['steps'])


# ---- b. the reference agrees with what it is built from

@pytest.mark.parametrize('name', sorted(sw.CASES))
def test_every_unpruned_utterance_ends_as_the_offline_decode(name, oracle_lib):
  tr = sw.walk(name)
  params, beam = tr['params'], tr['beam']
  seen = {'plain': 0, 'primed': 0, 'committed': 0, 'dead': 0}
  for k, life in enumerate(tr['lives']):
    if life.pruned or not life.given:
      continue
    what = (name, k, life.slot)
    labels, score = life.end
    frames = np.array(life.given)
    if life.prefix is None:
      out = oracle.decode(params, [frames], beam, 1, 1)
      want = (out['labels'][0].tolist(), int(sw._bits(out['scores'])[0]))   # pylint: disable=protected-access
    else:
      out = primed_ref.primed_decode(params, frames, life.prefix, beam)
      want = ((out['labels'][0].tolist(), int(sw._bits(out['scores'])[0])) if len(out['scores'])   # pylint: disable=protected-access
              else ([-1] * len(frames), INF_BITS))
    if life.dead:   # a non-finite frame: +inf, and -1 for everything not yet committed (what was committed stays)
      done = life.ref.committed
      assert score == want[1] == INF_BITS and labels[done:] == want[0][done:] == [-1] * (len(frames) - done), what
      seen['dead'] += 1
      continue
    assert (labels, score) == want, what
    seen['primed' if life.prefix is not None else 'plain'] += 1
    seen['committed'] += life.ref.committed > 0
  if name == 'one_launch':
    assert seen['plain'] >= 1 and seen['committed'] >= 1, seen
  else:
    assert all(v >= 1 for v in seen.values()), seen


# ---- c. ... push by push

@pytest.mark.parametrize('name', sorted(sw.CASES))
def test_unpruned_utterances_follow_the_oracles_replay(name, oracle_lib):
  tr = sw.walk(name)
  params, beam, steps = tr['params'], tr['beam'], tr['steps']
  inf = [INF_BITS] * beam
  checked = commits = 0
  for k, life in enumerate(tr['lives']):
    if life.pruned or life.prefix is not None or life.bad or not life.given:
      continue
    rep = nbest_ref.replay(params, np.array(life.given), beam)
    ref = commit_ref.ReplaySession(rep)
    for step, kind, arg in life.events:
      what = (name, k, life.slot, step)
      if kind == 'push':
        ref.push(arg)
      else:
        assert ref.commit()[0] == arg, what
        assert len(arg) % 2 == 0, what
        commits += len(arg) > 0
      if not ref.received:   # (a commit before the utterance's first frame)
        continue
      col = steps[step]['snap'][life.slot]
      rows, scores = nbest_ref.nbest(rep, upto=ref.received)
      assert col['rows'] == rows.tolist() and col['labels'] == rows[0].tolist(), what
      assert col['beam'] == (sw._bits(scores).tolist() + inf)[:beam] and col['scores'] == col['beam'][0], what   # pylint: disable=protected-access
      assert col['stable'] == ref.committed + nbest_ref.common_prefix(rows[:, ref.committed:]), what
      assert (col['received'], col['committed']) == (ref.have, ref.committed), what
    checked += 1
  assert checked >= 1, name
  if name in COMMITTING:
    assert commits >= 1, name


# ---- the trace keeps the contract's bookkeeping

@pytest.mark.parametrize('name', sorted(sw.CASES))
def test_the_traces_bookkeeping(name, oracle_lib):
  """Every commit hands out an even number of labels; what a restart hands out starts with what was committed; a
  restarted slot reads as a fresh one; nobody else changes at a restart, a prime or a refused call."""
  tr = sw.walk(name)
  n_utt, beam = tr['n_utt'], tr['beam']
  final = [[] for _ in range(n_utt)]
  for i, st in enumerate(tr['steps']):
    kind, res = st['kind'], st['result']
    touched = set(range(n_utt))
    if kind.startswith('commit'):
      for u in range(n_utt):
        assert len(res['labels'][u]) % 2 == 0, (name, i, u)
        final[u] += res['labels'][u]
        assert st['snap'][u]['committed'] == len(final[u]) and st['snap'][u]['labels'][:len(final[u])] == final[u], (name, i, u)
        assert st['snap'][u]['received'] == res['have'][u] - len(res['labels'][u]), (name, i, u)
        assert st['snap'][u]['received'] <= tr['max_frames']
    elif kind == 'restart':
      touched = set(res)
      for u in res:
        assert res[u]['labels'][:len(final[u])] == final[u] and res[u]['window'] == res[u]['labels'][len(final[u]):], (name, i, u)
        final[u] = []
        col = st['snap'][u]
        assert (col['labels'], col['rows'], col['counts'], col['stable'], col['received'], col['committed'], col['scores']) == \
               ([], [], 0, 0, 0, 0, 0), (name, i, u)
        assert col['beam'] == col['nb_scores'] == [INF_BITS] * beam, (name, i, u)
    elif kind == 'prime':
      touched = set(res)
      for u in res:
        col = st['snap'][u]
        assert col['counts'] == 1 and col['scores'] == res[u] and col['stable'] == col['received'] == len(st['call']['labels'][u]), (name, i, u)
    elif kind == 'refuse':
      touched = set()
    else:
      touched = {u for u in range(n_utt) if st['call']['chunks'][u] is not None}
    for u in set(range(n_utt)) - touched:
      assert st['snap'][u] == st['before'][u], (name, i, u)
