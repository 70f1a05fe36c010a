"""The random walks of tests/session_walk.py with the whole session replaced by its copy after every third operation:
OnlineSession.snapshot(), a new handle and a new session of the same shape, restore(), the old one closed.

The plans and their trace on the CPU reference are unchanged; every result and every snapshot the trace expects must
still hold exactly (tests/test_gpu_session_walk.py's comparisons).  What the walk may skip is capped, on the CPU,
before any device call: a slot that cannot be exported (its beam emptied by the plan's non-finite frame) is left fresh
by restore(), and that is allowed only where the trace's next operation on the slot is a restart or nothing; until
that restart the slot is not compared.  facts() also says which utterance states each case moves.

The one_launch plan has 17 operations in a window of 12 that it never fills: it is replayed at two phases (moves after
operations 0, 3, 6, ... and after 1, 4, 7, ...) and covers every state but the full window.  No plan retires or comes
near the cluster cap: those two states are tests/test_gpu_migrate.py's.
"""

import pytest

import session_walk as sw
import test_gpu_restart as gr
import test_gpu_session_walk as gw
from uisrnn_amd import _capi
from uisrnn_amd import uisrnn as host

pytestmark = pytest.mark.gpu

STATES = ('fresh', 'N1', 'N2', 'N3', 'N5', 'full', 'emptied', 'pruned', 'primed')
EVERY = 3


def facts(tr, phase):
  """From the trace alone: the states of the slots at every move (a move follows operation i where i % EVERY ==
  phase), and the slots a move leaves behind."""
  steps, n_utt, beam, window = tr['steps'], tr['n_utt'], tr['beam'], tr['max_frames']
  moved = {s: 0 for s in STATES}
  left, wrong = set(), []
  for i, st in enumerate(steps):
    if i % EVERY != phase:
      continue
    for u in range(n_utt):
      col = st['snap'][u]
      if col['received'] > 0 and col['counts'] == 0:   # an emptied beam: there is nothing to move
        later = [k for j, k in sw.slot_kinds(tr, u) if j > i and not k.startswith('commit')]
        left.add(u)
        if later and later[0] != 'restart':
          wrong.append((i, u, later[0]))
        continue
      have = col['received']
      moved['fresh'] += have == 0 and col['committed'] == 0
      for n in (1, 2, 3, 5):
        moved['N{}'.format(n)] += have == n
      moved['full'] += have == window
      moved['emptied'] += have == 0 and col['committed'] > 0
      moved['pruned'] += have > 0 and col['committed'] > 0 and 0 < col['counts'] < beam
      moved['primed'] += sw._last_kind(tr, u, i + 1) == 'prime'   # pylint: disable=protected-access
  killed = {st['op'][2] for st in steps if st['kind'] == 'push' and len(st['op']) > 2}
  return {'moved': moved, 'left': left, 'wrong': wrong, 'killed': killed}


def _check_facts(name, phases, missing=()):
  tr = sw.walk(name)
  total = {s: 0 for s in STATES}
  for phase in phases:
    f = facts(tr, phase)
    assert not f['wrong'], (name, phase, f['wrong'])          # a slot left fresh is restarted before anything else
    assert f['left'] <= f['killed'], (name, phase, f)         # ... and only the slots the plan kills are
    for s in STATES:
      total[s] += f['moved'][s]
  assert {s for s in STATES if not total[s]} == set(missing), (name, total)


def _online(dec, n_utt, beam, final):
  """An OnlineSession around an open session of `dec` (its committed labels: `final`): snapshot() and restore()."""
  session = host.OnlineSession.__new__(host.OnlineSession)
  session._decoder, session._num_utterances, session._beam_size = dec, n_utt, beam   # pylint: disable=protected-access
  session._final, session._open = final, True                                        # pylint: disable=protected-access
  return session


def _replay(name, path, phase):
  """test_gpu_session_walk._replay with the session replaced by its copy after every operation i, i % EVERY == phase."""
  tr, case = sw.walk(name), sw.CASES[name]
  n_utt, beam = case['n_utt'], case['beam']
  begin = lambda d: d.stream_begin(n_utt, beam, case['window'], max_clusters=case['cap'], flags=gw.PATHS[path])   # pylint: disable=unnecessary-lambda-assignment
  dec = _capi.Decoder(tr['params'])
  begin(dec)
  left, moves, exported = set(), 0, 0
  try:
    session = gr._Session(dec, n_utt, beam)   # pylint: disable=protected-access
    for i, st in enumerate(tr['steps']):
      what = (name, path, phase, 'step', i, st['op'])
      kind, call, want = st['kind'], st['call'], st['result']
      if kind == 'push':
        dec.stream_push(call['chunks'])
      elif kind in ('commit_none', 'commit_h'):
        got = session.commit(call['horizons'])
        for u in range(n_utt):
          assert (got[0][u], got[1][u]) == (want['labels'][u], want['dropped'][u]), what + ('slot', u)
      elif kind == 'restart':
        got, status = session.restart({u for u in range(n_utt) if call['which'][u]})
        assert status == _capi.UIS_OK and sorted(got) == sorted(want), what
        for u in want:
          if u in left:
            left.discard(u)      # (what a dead slot would have handed out stayed behind at the move)
          else:
            assert got[u] == want[u], what + ('slot', u)
      elif kind == 'prime':
        scores = dec.stream_prime(call['chunks'], call['labels'])
        for u in range(n_utt):
          assert int(gr._bits(scores)[u]) == want.get(u, 0), what + ('slot', u)   # pylint: disable=protected-access
      else:
        with pytest.raises(_capi.HipLibraryError) as err:
          if call['call'] == 'push':
            dec.stream_push(call['chunks'])
          else:
            dec.stream_prime(call['chunks'], call['labels'])
        assert err.value.status == want, what
      if i % EVERY == phase:   # ---- the whole session moves
        states = _online(dec, n_utt, beam, session.final).snapshot()
        for u in range(n_utt):
          col = st['snap'][u]
          dead = col['received'] > 0 and col['counts'] == 0
          assert (states[u] is None) == dead or u in left, what + ('slot', u)
        new = _capi.Decoder(tr['params'])
        begin(new)
        copy = _online(new, n_utt, beam, [[] for _ in range(n_utt)])
        copy.restore(states)
        dec.stream_end()
        dec.close()
        dec = new
        session = gr._Session(dec, n_utt, beam)   # pylint: disable=protected-access
        session.final = copy._final               # pylint: disable=protected-access
        left |= {u for u in range(n_utt) if states[u] is None}
        moves += 1
        exported += sum(1 for s in states if s is not None)
      shot = session.snapshot()
      assert shot['status'] == (_capi.UIS_OK, _capi.UIS_OK), what
      shot['received'], shot['committed'] = dec.stream_received().tolist(), dec.stream_committed().tolist()
      for u in range(n_utt):
        if u in left:
          continue
        for key in gw.KEYS:
          assert shot[key][u] == st['snap'][u][key], what + ('slot', u, key)
  finally:
    dec.stream_end()
    dec.close()
  assert moves == len(range(phase, len(tr['steps']), EVERY)) and exported > moves
  return left


def test_small(oracle_lib):
  _check_facts('small4', (0,))
  for path in ('default', 'stepwise'):
    _replay('small4', path, 0)


def test_deep(oracle_lib):
  _check_facts('deep', (0,))
  for path in ('default', 'stepwise'):
    _replay('deep', path, 0)


def test_embedded(oracle_lib):
  _check_facts('embedded', (0,))
  for path in ('default', 'stepwise', 'resident'):
    _replay('embedded', path, 0)


def test_one_launch(oracle_lib):
  _check_facts('one_launch', (0, 1), missing=('full',))
  for path in ('default', 'resident'):
    for phase in (0, 1):
      _replay('one_launch', path, phase)
