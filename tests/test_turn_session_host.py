"""Minimum turn length in streaming sessions, the CPU side: the reference of tests/turn_session_ref.py against the
references it is built from, the facts the GPU cases of tests/test_gpu_turn_session.py rely on, the Python front end's
keyword checks against a stand-in decoder, and csrc/uis_blob.h's validator and import normalisation on blobs with runs
(stand-alone, also under the host compiler's sanitizers).  No GPU needed.
"""

import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import known_ref
import known_session_ref as ksr
import test_restart_host as rh
import turn_ref
import turn_session_cases as tc
import turn_session_ref as tsr
import turn_walk
import uisrnn_amd
from uisrnn_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _final(name, plan):
  return tc.trace(name, plan)[-1]['snap']


def _strip(snap):
  return [{k: v for k, v in col.items() if k != 'm'} for col in snap]


# ---- 1. the reference against the references it is built from

@pytest.mark.parametrize('name', ['small4', 'deep'])
def test_without_a_rule_and_with_zeros_and_ones_it_is_the_session_without_one(name, oracle_lib):
  sh = tc.shape(name)
  plain, ones = _final(name, 'plain'), _final(name, 'zeros_ones')
  assert _strip(plain) == _strip(ones)
  for u, n in enumerate(tc.chunk_lengths(sh)):
    seq = sh.pool[u][0][0][:n]
    ref = ksr.Session(sh.model, sh.beam)
    for t0 in range(0, n, 3):
      ref.push(seq[t0:t0 + 3])
    assert ref.rows().tolist() == plain[u]['rows'] and _bits(ref.scores()).tolist() == plain[u]['scores'], (name, u)
    assert plain[u]['turns'] == [plain[u]['rows'][0][-1], 0] and all(run == 0 for _, run in plain[u]['words'])
    assert ones[u]['turns'][1] == 0 and all(run == 0 for _, run in ones[u]['words'])


@pytest.mark.parametrize('name', tc.SHAPES)
def test_in_every_chunking_it_is_the_offline_decode_under_the_rule(name, oracle_lib):
  sh = tc.shape(name)
  values = tc.slot_values(sh.n_utt)
  snaps = {kind: _final(name, 'chunk_' + kind) for kind in tc.CHUNKINGS}
  for kind in tc.CHUNKINGS:
    assert snaps[kind] == snaps['whole'], (name, kind)
  for u, n in enumerate(tc.chunk_lengths(sh)):
    want = turn_ref.decode(sh.model, sh.pool[u][0][0][:n], sh.beam, m=values[u])
    col = snaps['whole'][u]
    assert col['rows'] == [h.trace for h in want['beam']] and col['scores'] == _bits([h.score for h in want['beam']]).tolist()
    assert col['turns'] == [want['beam'][0].last, min(turn_ref.run(want['beam'][0].trace), values[u]) if values[u] >= 2 else 0]
    assert col['words'] == [[h.last, min(turn_ref.run(h.trace), values[u]) if values[u] >= 2 else 0] for h in want['beam']]
    assert all(turn_ref.rule_holds(row, values[u]) for row in col['rows']), (name, u)


@pytest.mark.parametrize('name', tc.SHAPES)
def test_the_rule_bites_on_every_shape_the_device_tests_use(name, oracle_lib):
  """m = 3 on every slot changes some slot's labels against the session without a rule, empties no beam and keeps every K
  under the cap -- and so do the per-slot values the device tests decode under.  tc.SEEDS is the first seed of 0 .. 8
  for which both hold; every shape has one."""
  sh = tc.shape(name)
  changed, emptied, most = tc.bites(name)
  assert changed and not emptied and most < sh.cap, (name, changed, emptied, most)
  free, mixed = _final(name, 'free'), _final(name, 'chunk_whole')
  values = tc.slot_values(sh.n_utt)
  assert any(mixed[u]['rows'][0] != free[u]['rows'][0] for u in range(sh.n_utt) if values[u] >= 2), name
  assert all(mixed[u]['rows'] == free[u]['rows'] and mixed[u]['scores'] == free[u]['scores'] for u in range(sh.n_utt) if values[u] < 2)
  assert all(col['live'] > 0 and col['K'] < sh.cap for col in mixed)
  for seed in range(tc.SEEDS[name]):   # (the seed is the FIRST: the earlier ones miss one of the two)
    c, e, k = tc.bites(name, seed)
    whole = tc.trace(name, 'chunk_whole', seed)[-1]['snap']
    other = tc.trace(name, 'free', seed)[-1]['snap']
    assert not (c and not e and k < sh.cap and any(whole[u]['rows'][0] != other[u]['rows'][0] for u in range(sh.n_utt))), seed


@pytest.mark.parametrize('plan', ['commit', 'restart', 'prime', 'retire'])
@pytest.mark.parametrize('name', tc.SHAPES)
def test_no_plan_empties_a_beam_or_reaches_the_cap(name, plan, oracle_lib):
  sh = tc.shape(name)
  tr = tc.trace(name, plan)
  for st in tr:
    for u, col in enumerate(st['snap']):
      assert col['K'] < sh.cap and (col['live'] > 0 or col['have'] + col['committed'] == 0), (plan, st['op'], u)
      assert all((run >= 1) == (col['m'] >= 2) and run <= max(col['m'], 0) for _, run in col['words'])
  if plan == 'commit':
    emptied = tr[6]
    assert emptied['kind'] == 'commit' and all(col['have'] == 0 and col['live'] == 1 for col in emptied['snap'])
    ruled = [u for u, col in enumerate(emptied['snap']) if col['m'] >= 2]
    assert ruled and all(emptied['snap'][u]['turns'][1] >= 1 for u in ruled)       # the run survives the emptied window
    # ... and some hypothesis is held by it afterwards: run < m at the commit, the same label at the next frame
    held = [u for u in ruled if emptied['snap'][u]['turns'][1] < emptied['snap'][u]['m']]
    for u in held:
      assert tr[7]['snap'][u]['rows'][0][-1] == emptied['snap'][u]['turns'][0]
  if plan == 'restart':
    assert tr[2]['snap'][2]['turns'] == [-1, 0] and tr[2]['snap'][2]['m'] == 3 and tr[3]['snap'][2]['turns'][1] >= 1
    assert tr[5]['snap'][2]['m'] == 5 and tr[6]['snap'][2]['turns'][1] >= 1


@pytest.mark.parametrize('name', tc.SHAPES)
def test_the_together_case_empties_slot_2_and_no_other(name, oracle_lib):
  sh = tc.shape(name)
  tr = tc.trace(name, 'together')
  assert tr[0]['call']['values'][2] == 3
  assert tr[2]['snap'][2]['live'] == 0 and tr[2]['snap'][2]['have'] == 2 and tr[2]['snap'][2]['turns'] == [-1, 0]
  assert tr[-1]['snap'][2]['live'] == 0 and tr[-1]['snap'][2]['have'] > 2
  assert all(col['live'] > 0 and col['K'] <= 3 for u, col in enumerate(tr[-1]['snap']) if u != 2)
  pushes = [st for st in tr if st['kind'] == 'push']
  assert all(st['call']['speakers'] is not None and st['call']['bias'] is not None for st in pushes)
  assert sum(bool(st['call']['speakers'].any()) for st in pushes) >= 2


@pytest.mark.parametrize('name', tc.SHAPES)
def test_the_retire_case_holds_what_it_is_for(name, oracle_lib):
  tr = tc.trace(name, 'retire')
  primed, before, after = tr[1], tr[4], tr[6]
  assert primed['snap'][0]['turns'] == [2, 2] and primed['snap'][0]['words'] == [[2, 2]]
  assert before['kind'] == 'query' and before['result']['retirable'][0] == [0, 1]      # and NOT 2, whatever its run
  assert after['kind'] == 'query' and after['snap'][0]['turns'] == [0, 2] and after['result']['retirable'][0] == []
  # the hypothesis is held for one more frame, then free
  assert tr[7]['snap'][0]['rows'] == [[0]] and tr[7]['snap'][0]['turns'] == [0, 3] and tr[7]['snap'][0]['live'] == 1
  assert tr[8]['snap'][0]['live'] > 1


@pytest.mark.parametrize('name', tc.SHAPES)
def test_primed_it_continues_as_the_offline_decode_from_that_hypothesis(name, oracle_lib):
  sh = tc.shape(name)
  tr = tc.trace(name, 'prime')
  values = tr[0]['call']['values']
  for u, prefix in tc.PRIME_PREFIXES.items():
    n = len(prefix)
    assert tr[1]['snap'][u]['turns'] == [prefix[-1], tsr.trailing_run(prefix, values[u])]
    seq = sh.pool[u][0][0]
    start = tsr.primed(sh.model, seq[:n], np.array(prefix))
    want = _decode_from(sh, start, seq[n:n + 7], values[u])
    col = tr[-1]['snap'][u]
    assert col['rows'] == [h.trace for h in want] and col['scores'] == _bits([h.score for h in want]).tolist()
  assert not turn_ref.rule_holds(list(tc.PRIME_PREFIXES[0]), 3), 'no short turn inside the prefix'
  assert tr[2]['snap'][0]['rows'][0][-1] == 0 and tr[2]['snap'][0]['live'] == 1        # run 2 under m = 3: held


def _decode_from(sh, start, frames, m):
  """known_ref.decode from `start` with turn_ref's filter in force: the rule reads the whole trace, the prefix included."""
  with turn_ref._rule(int(m)):   # pylint: disable=protected-access
    return known_ref.decode(sh.model, frames, sh.beam, start=start)['beam']


def test_the_import_rule_and_the_override():
  assert tsr.last_word(-1, 0, 3) == (-1, 0)
  assert tsr.last_word(4, 2, 0) == (4, 0) and tsr.last_word(4, 2, 1) == (4, 0)
  assert tsr.last_word(4, 0, 3) == (4, 3) and tsr.last_word(4, 5, 3) == (4, 3) and tsr.last_word(4, 2, 3) == (4, 2)
  assert tsr.trailing_run([0, 0, 1, 1, 1, 1], 3) == 3 and tsr.trailing_run([0, 1], 3) == 1 and tsr.trailing_run([0, 0], 0) == 0


@pytest.mark.parametrize('name', ['small4', 'deep'])
def test_an_import_decodes_on_under_the_target_slots_value(name, oracle_lib):
  sh = tc.shape(name)
  seq = sh.pool[2][0][0]
  src = tsr.Session(sh.model, sh.beam, m=5)
  src.push(seq[:7])
  # the same value: the copy and the source stay one
  twin = tsr.Session(sh.model, sh.beam, m=5).imported(src)
  assert twin.exported() == src.exported()
  # into a slot without a rule: bare labels, and from there the session without a rule
  bare = tsr.Session(sh.model, sh.beam, m=0).imported(src)
  assert all(run == 0 for _, run in bare.exported()) and [w[0] for w in bare.exported()] == [w[0] for w in src.exported()]
  free = ksr.Session(sh.model, sh.beam)
  free.beam = [h.copy() for h in src.beam]
  free.received = src.received
  # from a slot without a rule into m = 3: run 3, nothing is held; from m = 5 into m = 3: clamped
  loose = tsr.Session(sh.model, sh.beam, m=3).imported(bare)
  assert all(run == 3 for _, run in loose.exported())
  clamped = tsr.Session(sh.model, sh.beam, m=3).imported(src)
  assert [run for _, run in clamped.exported()] == [min(run, 3) for _, run in src.exported()]
  for s in (src, twin, bare, free, loose, clamped):
    s.push(seq[7:12])
  assert twin.rows().tolist() == src.rows().tolist() and _bits(twin.scores()).tolist() == _bits(src.scores()).tolist()
  assert bare.rows().tolist() == free.rows().tolist() and _bits(bare.scores()).tolist() == _bits(free.scores()).tolist()
  # (what follows the import obeys the rule; the turn that was under way when it arrived is free to end at once)
  assert all(n >= 3 for row in loose.rows().tolist() for n in turn_ref.turns(row[7:])[1:-1])


def test_the_walk_reaches_what_it_is_for(oracle_lib):
  """policy_walk's small plan under slot values (tests/turn_walk.py): the operations interleave under the rule."""
  steps = turn_walk.trace()
  sh = turn_walk.shape()
  assert sh.plan == turn_walk.pw.PLANS['small'](6, 16, 6, 3)   # the plan is policy_walk's, as it is
  facts = turn_walk.facts(steps)
  assert facts['kinds'] == ['commit', 'limits', 'move', 'move_refused', 'prime', 'push', 'refuse', 'restart', 'retire', 'setm']
  refusals = {st['op'][1] for st in steps if st['kind'] == 'refuse'}
  assert {'push', 'prime_received', 'prime_long', 'bias_length', 'bias_push_long', 'bias_value', 'limits_range'} <= refusals
  assert facts['held_after_commit'] and facts['held_pushes'] and facts['retired_under_rule'] and facts['primed_under_rule']
  assert facts['limits_changed_mid_stream'] and facts['dead']
  # moves cross values: a clamp (5 -> 3), an arrival without a run under a rule (0 -> 3), a rule dropped (5 -> 0)
  assert {(5, 3), (0, 3), (5, 0)} <= facts['crossings'] and facts['clamped_or_loosened'] >= 2
  assert sum(len(v) == 4 for v in facts['values_seen']) >= 4          # slots decode their utterances under every value in turn
  assert any(st['kind'] == 'push' and st['call']['pending'] for st in steps)
  assert max(col['K'] for st in steps for col in st['snap']) < turn_walk.MAX_CLUSTERS
  for st in steps:
    for col in st['snap']:
      assert all((run >= 1) == (col['m'] >= 2) and run <= col['m'] for _, run in col['words']), st['op']


# ---- 2. the front end, against a stand-in decoder

class _Turned(rh._StandIn):   # pylint: disable=protected-access
  """test_restart_host's stand-in with the slots' values and the library's fresh-slot rule."""

  def __init__(self, n_utt):
    super().__init__(n_utt)
    self.values = [0] * n_utt
    self.calls = []

  def session_set_min_turn(self, values):
    values = [int(v) for v in values]
    assert len(values) == len(self.values)
    self.calls.append(values)
    for u, v in enumerate(values):
      if v != self.values[u] and self.have[u] + self.done[u]:
        raise _capi.HipLibraryError('uis_session_min_turn: utterance {} has already received frames'.format(u))
    self.values = values

  def session_min_turn(self):
    return np.array(self.values, dtype=np.int32)

  def session_turns(self):
    return np.array([[-1, 0] if not self.have[u] else [int(self.have[u]) - 1, min(int(self.have[u]), self.values[u]) if self.values[u] >= 2 else 0]
                     for u in range(len(self.have))], dtype=np.int32)


def _session(n_utt):
  session = rh._session(n_utt, 100)   # pylint: disable=protected-access
  session._decoder = _Turned(n_utt)   # pylint: disable=protected-access
  return session


def test_the_session_keywords():
  s = _session(3)
  dec = s._decoder   # pylint: disable=protected-access
  assert s.min_turn() == [0, 0, 0]
  s.set_min_turn(3)
  assert s.min_turn() == [3, 3, 3] and dec.calls[-1] == [3, 3, 3]
  s.set_min_turn([0, 1, 5])
  assert s.min_turn() == [0, 1, 5]
  s.set_min_turn(None)
  assert s.min_turn() == [0, 0, 0]
  s.set_min_turn([0, 2, 3])
  n_calls = len(dec.calls)
  for bad, kind, match in ((True, ValueError, 'not a bool'), (-1, ValueError, 'must be in'), (32768, ValueError, 'must be in'),
                           (2.0, TypeError, 'must be an integer'), ([1, 2], ValueError, '2 entries for 3 utterances'),
                           ([1, 2, None], TypeError, 'must be an integer')):
    with pytest.raises(kind, match=match):
      s.set_min_turn(bad)
  assert len(dec.calls) == n_calls and s.min_turn() == [0, 2, 3]       # before any device work; nothing changed
  assert s.turns() == [(-1, 0, False)] * 3
  s.push([np.zeros((2, 4)), np.zeros((1, 4)), np.zeros((5, 4))])
  assert s.turns() == [(1, 0, False), (0, 1, True), (4, 3, False)]
  # the fresh-slot rule is the library's: the refusal comes through, the same table is accepted
  with pytest.raises(_capi.HipLibraryError):
    s.set_min_turn([0, 3, 3])
  s.set_min_turn([0, 2, 3])
  s.restart([1])
  s.set_min_turn([0, 3, 3])
  assert s.min_turn() == [0, 3, 3]


def test_turns_go_through_the_retired_id_map():
  s = _session(2)
  s.set_min_turn([3, 0])
  s.push([np.zeros((3, 4)), np.zeros((3, 4))])
  s._gone = [[0, 1], []]   # pylint: disable=protected-access  (two ids retired in slot 0: index 2 is id 4)
  assert s.turns() == [(4, 3, False), (2, 0, False)]


def test_the_pool_sets_a_slots_value_when_it_opens_a_stream():
  session = _session(3)
  pool = uisrnn_amd.uisrnn.StreamPool(session)
  a = pool.open('a', min_turn=3)
  b = pool.open('b')
  assert session.min_turn()[a] == 3 and session.min_turn()[b] == 0
  pool.push({'a': np.zeros((2, 4)), 'b': np.zeros((1, 4))})
  pool.finish('a')
  again = pool.open('c')                 # None keeps the slot's value
  assert again == a and session.min_turn()[a] == 3
  pool.finish('c')
  assert pool.open('d', min_turn=0) == a and session.min_turn()[a] == 0     # 0 is a value, not "keep"
  for bad, kind in ((True, ValueError), (-2, ValueError), (1.5, TypeError)):
    with pytest.raises(kind):
      pool.open('e', min_turn=bad)
  assert 'e' not in pool._slot   # pylint: disable=protected-access


def test_the_model_entries_check_min_turn_before_any_device_work():
  model_args, _, inference_args = uisrnn_amd.parse_arguments([])
  model_args.observation_dim = 4
  model = uisrnn_amd.UISRNN(model_args)
  inference_args.look_ahead, inference_args.test_iteration = 1, 1
  for call in (lambda **kw: model.online(2, inference_args, 10, **kw), lambda **kw: model.online_pool(2, inference_args, 10, **kw),
               lambda **kw: model.predict_primed([np.zeros((3, 4))] * 2, [[0], [0]], inference_args, **kw)):
    for bad, kind in ((True, ValueError), ([1], ValueError), (-1, ValueError), ('3', TypeError)):
      with pytest.raises(kind, match='min_turn'):
        call(min_turn=bad)


# ---- 3. the blob validator and the import normalisation, stand-alone

def _build_blob_turn(tmp_path, flags):
  cxx = shutil.which(os.environ.get('CXX', '') or 'g++') or shutil.which('c++') or shutil.which('clang++')
  if not cxx:
    pytest.skip('no host C++ compiler')
  exe = str(tmp_path / 'blob_turn')
  subprocess.run([cxx] + flags + ['-I', os.path.join(ROOT, 'uisrnn_amd', 'csrc'), os.path.join(ROOT, 'tests', 'blob_turn_main.cpp'),
                                  '-o', exe], check=True)
  return exe


def test_the_blob_validator_and_the_import_normalisation(tmp_path):
  exe = _build_blob_turn(tmp_path, ['-std=c++17', '-O1', '-Wall', '-Wextra'])
  path = str(tmp_path / 'runs.blob')
  done = subprocess.run([exe, path], capture_output=True, text=True)
  assert done.returncode == 0 and done.stdout.startswith('blob_turn: ok'), (done.returncode, done.stdout, done.stderr)
  with open(path, 'rb') as f:
    blob = f.read()
  assert _capi.blob_info(blob)['K'] == 3 and _capi.blob_max_tag(blob) == 0   # (the Python helpers read it as before)


def test_the_same_under_the_host_compilers_sanitizers(tmp_path):
  cxx = shutil.which(os.environ.get('CXX', '') or 'g++') or shutil.which('c++') or shutil.which('clang++')
  if not cxx:
    pytest.skip('no host C++ compiler')
  base = ['-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
  probe = str(tmp_path / 'probe.cpp')
  with open(probe, 'w') as f:
    f.write('int main() { return 0; }\n')
  # (as tests/test_migrate_host.py builds blob_check_main.cpp: the runtime inside the program where the compiler offers that)
  for flags in (base + ['-static-libasan', '-static-libubsan'], base + ['-static-libsan'], base):
    if subprocess.run([cxx] + flags + [probe, '-o', str(tmp_path / 'probe')], capture_output=True).returncode == 0:
      break
  else:
    pytest.skip('the host compiler cannot link the sanitizer runtime')
  if subprocess.run([str(tmp_path / 'probe')], capture_output=True).returncode != 0:
    pytest.skip('a program with the sanitizer runtime does not start in this environment')
  exe = _build_blob_turn(tmp_path, flags)
  done = subprocess.run([exe], capture_output=True, text=True)
  assert done.returncode == 0 and done.stdout.startswith('blob_turn: ok'), (done.returncode, done.stdout, done.stderr)


# ---- 4. the C ABI's surface

def test_the_symbols_are_declared_and_begin_with_neither_reserved_prefix():
  names = ('uis_session_min_turn', 'uis_session_get_min_turn', 'uis_session_turns')
  assert set(names) <= set(_capi.EXPORTED_SYMBOLS) and _capi.UIS_ABI_VERSION == 6
  with open(os.path.join(ROOT, 'include', 'uisrnn_hip.h')) as f:
    header = f.read()
  for name, args in (('uis_session_min_turn', r'uis_handle\* h, const int32_t\* min_turn'),
                     ('uis_session_get_min_turn', r'uis_handle\* h, int32_t\* out'),
                     ('uis_session_turns', r'uis_handle\* h, int32_t\* out')):
    assert re.search(r'int32_t {}\({}'.format(name, args), header), name
    assert not name.startswith(('uis_stream_', 'uis_decode'))
  assert 'a session never holds a run' not in header


def test_the_calls_refuse_a_null_handle():   # (the refusal without a session, on a live handle: tests/test_gpu_turn_session.py)
  lib = _capi.load_library()
  for name in ('uis_session_min_turn', 'uis_session_get_min_turn', 'uis_session_turns'):
    assert getattr(lib, name)(None, None) == _capi.UIS_ERR_INVALID_ARG
