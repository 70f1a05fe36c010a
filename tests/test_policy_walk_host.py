"""The policy walks' CPU side (tests/policy_walk.py): no GPU needed.

  a. the reference adds nothing where the two rules are absent: a plan stripped of them is a session_walk plan, and
     its trace is session_walk.trace's, snapshot by snapshot; all-NaN and all-p0 tables trace as no tables, bit for bit
  b. the reference agrees with what it is built from: every utterance that was never committed, retired, moved or
     primed and whose limit never changed ends with the labels and the beam scores of bias_ref.decode of its frames,
     its concatenated tables and its limit
  c. the plans reach the states they are meant for -- asserted on the reference's trace alone, as counts
"""

import numpy as np
import pytest

import bias_ref
import policy_walk as pw
import primed_ref
import session_walk as sw

TABLED = ('small4', 'small10', 'deep', 'embedded', 'one_launch')   # limits_only is one_launch's script without tables
FULL = ('small4', 'small10', 'deep', 'embedded')                    # the plans with a body
TABLE_REFUSALS = ('bias_length', 'bias_push_long', 'bias_prime', 'limits_range', 'bias_value')


def _trace(name, plan, cap=None):
  case = pw.CASES[name]
  return pw.trace(pw.walk(name, True)['params'], pw.case_pools(name), case['beam'], case['window'], plan,
                  case['cap'] if cap is None else cap)


# ---- a. nothing new where the rules are absent

@pytest.mark.parametrize('name', sorted(pw.CASES))
def test_without_the_rules_the_trace_is_session_walks(name, oracle_lib):
  case = pw.CASES[name]
  plan = pw.strip(pw.case_plan(name))
  assert all(op[0] in ('push', 'commit', 'restart', 'prime', 'refuse') and len(op) <= 4 for op in plan)
  params = pw.walk(name, True)['params']
  # (a cap that neither reference comes near: session_walk keeps the cap outside its model, and nothing steers)
  want = sw.trace(params, pw.case_pools(name), case['beam'], case['window'], plan, 64)
  got = _trace(name, plan, cap=64)
  assert [st['op'] for st in got['steps']] == list(plan), 'the reference steered'
  assert len(want['steps']) == len(got['steps'])
  for i, (a, b) in enumerate(zip(want['steps'], got['steps'])):
    assert (a['kind'], a['result']) == (b['kind'], b['result']), (name, i, a['op'])
    for u in range(case['n_utt']):
      assert a['snap'][u] == {k: b['snap'][u][k] for k in a['snap'][u]}, (name, i, a['op'], u)
      assert b['snap'][u]['limit'] == 0


@pytest.mark.parametrize('name', TABLED)
def test_null_tables_trace_as_no_tables(name, oracle_lib):
  plan = pw.case_plan(name)
  base = _trace(name, pw.retable(plan, 'none'))
  assert all(st['call']['bias'] is None for st in base['steps'] if st['kind'] == 'push')
  for kind in ('nan', 'p0'):
    other = _trace(name, pw.retable(plan, kind))
    assert sum(st['call']['bias'] is not None for st in other['steps'] if st['kind'] == 'push') >= 5
    assert len(other['steps']) == len(base['steps'])
    for i, (a, b) in enumerate(zip(base['steps'], other['steps'])):
      assert (a['kind'], a['result'], a['snap']) == (b['kind'], b['result'], b['snap']), (name, kind, i, a['op'])


# ---- b. the reference agrees with the offline decode

@pytest.mark.parametrize('name', sorted(pw.CASES))
def test_every_untouched_utterance_ends_as_the_offline_decode(name, oracle_lib):
  tr = pw.walk(name, True)
  model, beam = primed_ref.Model(tr['params']), tr['beam']
  seen = {'plain': 0, 'bounded': 0, 'tabled': 0, 'both': 0, 'dead': 0}
  for k, life in enumerate(pw.offline_lives(tr)):
    tables = np.array(life.tables, dtype=np.float64)
    with np.errstate(all='ignore'):
      out = bias_ref.decode(model, np.array(life.given), beam, 1, 1, limit=life.limit0, bias=tables)
    col = life.end_col
    assert col['committed'] == 0 and col['received'] == len(life.given), (name, k)
    assert col['labels'] == out['labels'].tolist(), (name, k, life.slot)
    assert col['beam'] == sw._bits(out['beam_scores']).tolist(), (name, k, life.slot)   # pylint: disable=protected-access
    assert col['rows'] == [h.trace for h in out['beam']], (name, k, life.slot)
    tabled, bounded = bool(np.isfinite(tables).any()), life.limit0 > 0
    seen[('plain', 'bounded', 'tabled', 'both')[2 * tabled + bounded]] += 1
    seen['dead'] += not out['beam']
  if name in FULL:   # some under a bound, some under a table, one that a contradiction emptied
    assert seen['bounded'] + seen['both'] >= 1 and seen['tabled'] + seen['both'] >= 1 and seen['dead'] >= 1, seen
  else:
    assert sum(seen.values()) >= 1, seen


# ---- c. the plans reach their states

def _limit_facts(name, f):
  # the bound bound: some hypothesis at K == limit, and the same step without the bound would have kept a new cluster
  assert f['bound_steps'] >= 5, f['bound_steps']
  # a limit lowered below a live K (facts() asserts that K never grew afterwards); a limit raised, and K grew past the
  # old value; a cluster opened again after a retirement at a slot whose K had equalled its limit
  assert f['lowered_below_K'] >= 1 and f['raised_and_grew'] >= 1 and f['reopened_after_retirement'] >= 1, f
  # a limit set to 0 on a slot whose K had reached it, after which K grew on
  assert f['lifted_and_grew'] >= 1, f
  # a bounded and an unbounded slot decode in one push; the reference steered an unbounded slot away from the cap
  # (not on `deep`: the toy model merges the speakers and its unbounded slots stay far below the cap)
  assert f['mixed_pushes'] >= 1 and (f['steered'] >= 1 or name == 'deep'), (f['mixed_pushes'], f['steered'])
  # a move between slots of different limits and window parities
  assert f['moves_between_limits'] >= 1 and f['moves_between_parities'] >= 1, f
  # a primed prefix of more clusters than the slot's limit, four frames or more behind it, and K never grew
  assert f['primed_above_the_limit'] >= 1, f
  assert all(f['kinds'][k] >= 1 for k in pw.OP_KINDS), f['kinds']
  assert all(v >= 1 for v in f['retire_modes'].values()) and f['retired'] >= 3, (f['retire_modes'], f['retired'])
  assert f['refusals_followed']
  if name.startswith('small'):
    # limit == cap: K reached the cap and the utterance received eight frames or more there (overflow stays 0)
    assert f['frames_at_the_cap'] >= 8, f['frames_at_the_cap']


@pytest.mark.parametrize('name', TABLED)
def test_the_plan_reaches_its_states(name, oracle_lib):
  tr = pw.walk(name, True)
  f = pw.facts(tr)
  _limit_facts(name, f)
  assert all(f['table_kinds'][k] >= 1 for k in pw.TABLE_KINDS), f['table_kinds']
  # every refusal in a session with committed frames and a wide beam
  wanted = TABLE_REFUSALS + ('push', 'prime_received', 'prime_long')
  assert all(f['refusals'].get(k, 0) >= 1 for k in wanted), f['refusals']
  assert all(st['call']['stays'] is not None for st in tr['steps'] if st['op'][:2] == ('refuse', 'bias_value'))
  # a table changed the labels of its push: three pushes, one of them by a 0 and one by a 1
  assert f['table_changed'] >= 3 and f['changed_by_0'] >= 1 and f['changed_by_1'] >= 1, f
  # the moved utterance's next push: its rows of the table behind a silent slot's
  assert f['moved_rows_behind_a_silent_slot'] >= 1
  # a commit with a positive horizon between two biased pushes of one utterance; a biased push behind a commit that
  # lengthened the prior tables
  assert f['commit_between_biased_pushes'] >= 1 and f['biased_push_after_the_tables_grew'] >= 1, f
  # both contradictions emptied a beam; the slot was restarted and held a full beam again
  assert all(v >= 1 for v in f['contradictions'].values()) and all(v >= 1 for v in f['revived'].values()), f
  # the budgets
  if name.startswith('small'):
    assert 100 <= f['operations'] <= 135 and 400 <= f['frames'] <= 600, (f['operations'], f['frames'])
  elif name in FULL:
    assert 50 <= f['operations'] <= 70, f['operations']
  else:
    assert f['frames'] <= 90, f['frames']


def test_the_plan_without_tables(oracle_lib):
  """limits_only: one_launch's script without its tables, for the path that takes none."""
  tr = pw.walk('limits_only', True)
  f = pw.facts(tr)
  _limit_facts('limits_only', f)
  assert f['frames'] <= 90
  assert f['refusals'] == {'limits_range': 1, 'bias_push_persistent': 1, 'push': 1, 'prime_received': 1, 'prime_long': 1}, f['refusals']
  tabled = [st for st in tr['steps'] if st['call'] and st['call'].get('bias') is not None]
  assert [st['op'][1] for st in tabled] == ['bias_push_persistent']
  a = [op for op in pw.case_plan('one_launch') if op[0] not in ('push', 'refuse')]
  b = [op for op in pw.case_plan('limits_only') if op[0] not in ('push', 'refuse')]
  assert [op for op in a if op != ('restart', (2,))] == [op for op in b if op != ('restart', (2,))]


@pytest.mark.parametrize('name', sorted(pw.CASES))
def test_the_traces_bookkeeping(name, oracle_lib):
  """A refused call, a query and a refused export change nothing; a limits call changes the limits alone; only the
  slots an operation names change; no hypothesis ever holds more clusters than the cap."""
  tr = pw.walk(name, True)
  n_utt = tr['n_utt']
  for i, st in enumerate(tr['steps']):
    kind = st['kind']
    if kind in ('refuse', 'move_refused') or (kind == 'retire' and not any(st['result']['retired'])):
      touched = set()
    elif kind == 'push':
      touched = {u for u in range(n_utt) if st['call']['chunks'][u] is not None}
    elif kind in ('restart', 'prime'):
      touched = set(st['result'])
    elif kind == 'move':
      touched = {st['call']['src'], st['call']['dst']}
    elif kind == 'retire':
      touched = {u for u in range(n_utt) if st['result']['retired'][u]}
    else:
      touched = set(range(n_utt))
    for u in set(range(n_utt)) - touched:
      assert st['snap'][u] == st['before'][u], (name, i, st['op'], u)
    if kind == 'limits':
      for u in range(n_utt):
        assert {k: v for k, v in st['snap'][u].items() if k != 'limit'} == {k: v for k, v in st['before'][u].items() if k != 'limit'}
    assert max(st['aux']['most']) <= tr['cap'] and all(c['overflow'] == 0 for c in st['snap']), (name, i)
