"""Minimum turn length on the CPU: the reference the GPU tests compare with, and the surface.

tests/turn_ref.py restates the beam search with one more filter in known_ref's candidates: a hypothesis whose last
label's run is below m keeps that label only.  With no table and with m = 0 or 1 it is oracle.decode bit for bit; on a
7-frame utterance with nothing pruned its final beam is exactly the brute-force set of labelings that satisfy the rule,
each at forced_ref's score; with m beyond the decode's length it is the all-zero labeling: that is what makes it a
reference.  Then the case table of the GPU sweep (m = 3 changes labels, empties no beam, stays inside every row's cap),
the keyword's checks and the regroupings of the Python front end, with the library stubbed as
tests/test_known_host.py does.  No GPU needed.
"""

import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import forced_ref
import golden_util
import instantiation_cases as ic
import known_ref
import turn_cases
import turn_ref
import uisrnn_amd
from uisrnn_amd import _capi
from uisrnn_amd import arguments
from uisrnn_amd import uisrnn as host

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM = 4


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _short(case, n_utt=2, frames=10):
  return [s[:frames] for s in case['seqs'][:n_utt]]


def test_the_helpers():
  assert [turn_ref.run(t) for t in ([], [0], [0, 0], [0, 1], [0, 1, 1, 1], [1, 0, 1])] == [0, 1, 2, 1, 3, 1]
  assert turn_ref.turns([0, 0, 1, 0, 0, 0]) == [2, 1, 3] and turn_ref.turns([]) == []
  assert turn_ref.rule_holds([0, 0, 0, 1, 1, 1, 2], 3) and not turn_ref.rule_holds([0, 0, 1, 1, 1], 3)
  assert known_ref.candidates is turn_ref._known_candidates   # pylint: disable=protected-access


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2', 'd20_h24_depth3'])
@pytest.mark.parametrize('look_ahead', [1, 2, 3])
@pytest.mark.parametrize('test_iteration', [1, 2])
def test_without_a_rule_it_is_the_oracle_decode(name, look_ahead, test_iteration, oracle_lib):
  case = golden_util.load_case(name)
  seqs = _short(case, 2, 10 if look_ahead < 3 else 7) + [case['seqs'][-1][:1]]
  beam = 4 if look_ahead < 3 else 3
  ref = oracle_lib.decode(case['params'], seqs, beam, look_ahead, test_iteration, n_threads=2)
  for what, ms in (('no table', None), ('zeros', [0] * len(seqs)), ('ones', [1] * len(seqs))):
    got = turn_ref.decode_list(case['params'], seqs, beam, look_ahead, test_iteration, ms=ms)
    for u in range(len(seqs)):
      assert np.array_equal(got['labels'][u], ref['labels'][u]), (what, u)
    assert np.array_equal(_bits(got['scores']), _bits(ref['scores'])), what
    assert np.array_equal(_bits(got['beam_scores']), _bits(ref['beam_scores'])), what
    assert np.array_equal(got['max_clusters'], ref['max_clusters']), what


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2', 'd20_h24_depth3'])
@pytest.mark.parametrize('look_ahead', [1, 2, 3])
@pytest.mark.parametrize('test_iteration', [1, 2])
def test_the_rule_holds_in_every_hypothesis(name, look_ahead, test_iteration, oracle_lib):
  """Every completed turn of every surviving hypothesis' FULL trace (both passes, the run across the pass boundary) has
  at least m steps -- and somewhere a turn is completed at all."""
  case = golden_util.load_case(name)
  completed = 0
  for m in (2, 3, 5):
    for seq in _short(case, 3, 12 if look_ahead < 3 else 8):
      beam = 4 if look_ahead < 3 else 3
      got = turn_ref.decode(case['params'], seq, beam, look_ahead, test_iteration, m=m)
      assert got['beam'], 'the rule alone cannot empty a beam'
      for hyp in got['beam']:
        assert len(hyp.trace) == test_iteration * len(seq)
        assert turn_ref.rule_holds(hyp.trace, m), (m, hyp.trace)
        completed += len(turn_ref.turns(hyp.trace)) > 1
  assert completed


def _growth_strings(n, limit):
  """Every restricted-growth labeling of n frames with at most `limit` labels."""
  out = []

  def grow(prefix, k):
    if len(prefix) == n:
      out.append(tuple(prefix))
      return
    for c in range(min(k + 1, limit)):
      grow(prefix + [c], max(k, c + 1))

  grow([], 0)
  return out


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2'])
@pytest.mark.parametrize('m', [2, 3])
@pytest.mark.parametrize('look_ahead', [1, 2, 3])
def test_nothing_pruned_it_is_the_brute_force_set_at_the_forced_scores(name, m, look_ahead, oracle_lib):
  """7 frames under max_speakers 3: 365 restricted-growth labelings, a beam of 400 prunes nothing.  The final beam is
  the set of those whose completed turns all have m frames or more, each at forced_ref.score_one's score."""
  case = golden_util.load_case(name)
  seq = case['seqs'][0][:7]
  every = _growth_strings(7, 3)
  assert len(every) == 365
  want = {lab for lab in every if turn_ref.rule_holds(lab, m)}
  assert 1 < len(want) < len(every)
  got = turn_ref.decode(case['params'], seq, 400, look_ahead, 1, limit=3, m=m)
  traces = [tuple(h.trace) for h in got['beam']]
  assert len(set(traces)) == len(traces) and set(traces) == want
  for hyp in got['beam']:
    score, _ = forced_ref.score_one(case['params'], seq, np.array(hyp.trace, dtype=np.int32))
    assert _bits(hyp.score) == _bits(score), hyp.trace


@pytest.mark.parametrize('look_ahead,test_iteration', [(1, 1), (1, 2), (2, 2), (3, 1)])
def test_a_large_m_is_one_speaker_at_the_forced_score(look_ahead, test_iteration, oracle_lib):
  case = golden_util.load_case('tiny_d16')
  seq = case['seqs'][1][:9]   # (without a rule its labels change speaker)
  total = test_iteration * len(seq)
  assert any(turn_ref.decode(case['params'], seq, 4, look_ahead, test_iteration)['labels'])
  score, _ = forced_ref.score_one(case['params'], np.tile(seq, (test_iteration, 1)), np.zeros(total, dtype=np.int32))
  for m in (total, total + 1, 32767):
    got = turn_ref.decode(case['params'], seq, 4, look_ahead, test_iteration, m=m)
    assert len(got['beam']) == 1 and got['beam'][0].trace == [0] * total
    assert got['labels'].tolist() == [0] * len(seq) and _bits(got['score']) == _bits(score)


def test_the_first_returned_turn_may_look_short_after_two_passes(oracle_lib):
  """test_iteration 2: the run continues across the pass boundary, so the returned labels (the last N steps) may open
  with the tail of a turn that began in the first pass."""
  case = golden_util.load_case('tiny_d16')
  short = 0
  for seq in _short(case, 3, 12):
    got = turn_ref.decode(case['params'], seq, 4, 1, 2, m=3)
    for hyp in got['beam']:
      assert turn_ref.rule_holds(hyp.trace, 3)
      tail = turn_ref.turns(hyp.trace[-len(seq):])
      short += len(tail) > 1 and tail[0] < 3
  assert short


def test_the_contradictions_empty_the_beam(oracle_lib):
  case = golden_util.load_case('tiny_d16')
  seq = case['seqs'][0][:8]
  n = len(seq)
  # two different tags on neighbouring frames under m = 3: at the start of the utterance, where the first turn is one
  # frame old, and later, where tag 9 opens a turn that tag 5 would have to end after one frame
  for two in ([5, 9, 0, 0, 0, 0, 0, 0], [5, 0, 0, 9, 5, 0, 0, 0]):
    two = np.array(two, dtype=np.uint8)
    for look_ahead in (1, 2, 3):
      got = turn_ref.decode(case['params'], seq, 4, look_ahead, 1, tags=two, m=3)
      assert not got['beam'] and got['labels'].tolist() == [-1] * n and np.isposinf(got['score'])
      assert turn_ref.decode(case['params'], seq, 4, look_ahead, 1, tags=two, m=1)['beam']
  # ... three frames apart they fit
  apart = np.array([0, 0, 5, 0, 0, 9, 0, 0], dtype=np.uint8)
  got = turn_ref.decode(case['params'], seq, 4, 1, 1, tags=apart, m=3)
  assert got['beam'] and all(h.trace[2] != h.trace[5] and turn_ref.rule_holds(h.trace, 3) for h in got['beam'])
  # a bias of 1 (change) one step into a turn
  change = np.full(n, np.nan)
  change[1:3] = 1.0
  assert not turn_ref.decode(case['params'], seq, 4, 1, 1, bias=change, m=3)['beam']
  assert turn_ref.decode(case['params'], seq, 4, 1, 1, bias=change)['beam']


# ---- the case table of the GPU sweep

_OFFLINE_ROWS = [row for row in ic.ROWS if not row[4]]


@pytest.mark.parametrize('row', _OFFLINE_ROWS, ids=[ic.row_id(row) for row in _OFFLINE_ROWS])
def test_the_case_table_bites(row, oracle_lib):
  """Every case of the sweep, at the utterances tests/test_gpu_turn.py compares (ncl = 8): its m empties no beam and
  keeps the survivors inside the case's cap, and it changes the labels of at least one compared utterance -- of every
  case but turn_cases.QUIET's, whose rows bite through their other cases."""
  bites = 0
  for listed in ic.CASES[row]:
    case, _, ms, free, ref = turn_cases.case_reference(listed, 8)
    assert case.row == row and case.name == listed.name
    changed = [u for u, r in ref.items() if not np.array_equal(free['labels'][u], r['labels'])]
    assert changed or case.name in turn_cases.QUIET, case.name
    bites += bool(changed)
    assert all(r['beam'] for r in ref.values()), case.name
    need = max(r['max_clusters'] for r in ref.values())
    assert need + case.look_ahead - 1 <= case.cap, (case.name, need, case.cap)
    for u, r in ref.items():
      assert all(turn_ref.rule_holds(h.trace, ms[u]) for h in r['beam']), (case.name, u)
  assert bites, row


def test_the_sweeps_own_table_names_cases_of_the_case_table():
  names = {case.name for row in _OFFLINE_ROWS for case in ic.CASES[row]}
  assert set(turn_cases.OTHER) <= names and set(turn_cases.QUIET) <= names and not set(turn_cases.OTHER) & set(turn_cases.QUIET)
  assert all(m in (2, 3, 5) and 0 <= seed <= 8 for seed, m in turn_cases.OTHER.values())


# ---- the surface

def test_the_new_symbol_is_declared_bound_and_exported():
  header = open(os.path.join(_ROOT, 'include', 'uisrnn_hip.h')).read()
  assert re.search(r'int32_t uis_min_turn\(uis_handle\* h, const int32_t\* min_turn, int32_t n_utt\);', header)
  assert 'uis_min_turn' in _capi.EXPORTED_SYMBOLS
  lib = _capi.load_library()
  assert lib.uis_min_turn.argtypes is not None
  assert lib.uis_min_turn(None, None, 0) == _capi.UIS_ERR_INVALID_ARG   # a null handle is refused, not dereferenced
  assert lib.uis_abi_version() == 6
  for fn in ('predict', 'predict_single', 'predict_nbest', 'predict_posteriors'):
    assert 'min_turn' in getattr(uisrnn_amd.UISRNN, fn).__code__.co_varnames, fn
  assert 'min_turn' in host.parallel_predict.__code__.co_varnames
  for fn in ('predict_primed', 'online', 'online_pool'):
    assert 'min_turn' not in getattr(uisrnn_amd.UISRNN, fn).__code__.co_varnames, fn
  for fn in ('decode', 'decode_f64', 'decode_host', 'decode_device'):
    assert 'min_turn' in getattr(_capi.Decoder, fn).__code__.co_varnames, fn


def test_the_keyword_as_the_librarys_table():
  check = host._check_min_turn  # pylint: disable=protected-access
  assert check(None, 3) is None
  # 0 and 1 mean no rule: a table of them is no table at all
  assert check(0, 3) is None and check(1, 3) is None and check([0, 1, 1], 3) is None and check([], 0) is None
  assert check(3, 2) == [3, 3] and check([0, 2, 32767], 3) == [0, 2, 32767]
  assert check(np.int64(4), 1) == [4] and check(np.array(4), 2) == [4, 4] and check(np.array([1, 5]), 2) == [1, 5]
  assert check((2, 0), 2) == [2, 0]
  for bad in (True, np.bool_(False), -1, 32768, [3, 3], [3, 3, 3, 3], [3, -1, 3], [3, 32768, 3], [3, True, 3],
              np.array([3, 3])):
    with pytest.raises(ValueError):
      check(bad, 3)
  for bad in (3.0, np.float32(2), '3', [3, 2.0, 3], [3, None, 3], [3, '3', 3], np.array([3.0, 3.0, 3.0])):
    with pytest.raises(TypeError):
      check(bad, 3)


def test_invalid_values_raise_before_any_device_work():
  model = uisrnn_amd.UISRNN(types.SimpleNamespace(
      observation_dim=4, rnn_hidden_size=8, rnn_depth=1, rnn_dropout=0.0, transition_bias=None, crp_alpha=1.0,
      sigma2=None, verbosity=0, enable_cuda=False))

  def no_device(*unused_args, **unused_kwargs):
    raise AssertionError('reached the device')

  model._get_decoder = no_device   # pylint: disable=protected-access
  model._decode_batch = no_device  # pylint: disable=protected-access
  args = types.SimpleNamespace(beam_size=4, look_ahead=1, test_iteration=1)
  seqs = [np.zeros((3, 4)), np.zeros((2, 4))]
  calls = (lambda m: model.predict(seqs, args, min_turn=m),
           lambda m: model.predict_nbest(seqs, args, min_turn=m),
           lambda m: model.predict_posteriors(seqs, args, min_turn=m),
           lambda m: host.parallel_predict(model, seqs, args, min_turn=m))
  for call in calls:
    for bad in (True, -1, 32768, [3], [3, 3, 3], [3, -2], [3, False]):
      with pytest.raises(ValueError):
        call(bad)
    for bad in (2.5, 3.0, '3', [3, 2.0]):
      with pytest.raises(TypeError):
        call(bad)
  for call in (lambda m: model.predict_single(seqs[0], args, min_turn=m), lambda m: model.predict(seqs[0], args, min_turn=m)):
    for bad in (True, -1, 32768, [3, 3]):
      with pytest.raises(ValueError):
        call(bad)
    with pytest.raises(TypeError):
      call(3.0)


# ---- the table follows the regroupings (stand-in decoders, as tests/test_known_host.py)

def _model(**inference):
  model_args, _, inference_args = arguments.parse_arguments([])
  model_args.observation_dim = DIM
  for key, value in inference.items():
    setattr(inference_args, key, value)
  return uisrnn_amd.UISRNN(model_args), inference_args


def _error(status, text):
  err = _capi.HipLibraryError('stand-in failed ({}): {}'.format(status, text))
  err.status = status
  return err


def _numbered(n_utt, need=()):
  """Utterance k: 3 + k % 4 frames, k in column 0, the level capacity it needs in column 1."""
  seqs = []
  for k in range(n_utt):
    s = np.zeros((3 + k % 4, DIM))
    s[:, 0] = k
    s[:, 1] = need[k] if k < len(need) else 100
    seqs.append(s)
  return seqs


def _turns(seqs):
  """Utterance k asks for 2 + k: the table says whose value it is."""
  return [2 + k for k in range(len(seqs))]


class _Regrouped:
  """decode_f64 that checks the min_turn table it is handed against the numbers of the sequences it is handed; at most
  `room` utterances per call; utterance k needs a level capacity of its column 1, and overflows a cluster cap below
  `cap_need[k]`."""

  def __init__(self, room=99, cap_need=None):
    self.room, self.cap_need, self.calls, self.flags = room, cap_need or {}, [], np.zeros(0, dtype=np.int32)

  def decode_f64(self, seqs, beam_size, look_ahead, test_iteration, max_clusters=0, flags=0, level_cap=0, **tables):
    cap = level_cap or 32768
    numbers = [int(s[0, 0]) for s in seqs]
    self.calls.append((numbers, cap, max_clusters))
    assert sorted(tables) == ['min_turn']
    assert tables['min_turn'] == [2 + k for k in numbers]
    if len(seqs) > self.room:
      self.flags = np.zeros(0, dtype=np.int32)
      raise _error(_capi.UIS_ERR_OOM, 'decode state would need 999 GB')
    self.flags = np.array([2 if int(s[0, 1]) > cap else 0 for s in seqs], dtype=np.int32)
    if self.flags.any():
      raise _error(_capi.UIS_ERR_UNSUPPORTED, 'a look-ahead window held more prefixes than a level')
    labels = np.concatenate([np.full(s.shape[0], k, dtype=np.int32) for s, k in zip(seqs, numbers)])
    overflow = np.array([1 if max_clusters < self.cap_need.get(k, 0) else 0 for k in numbers], dtype=np.int32)
    return {'status': 0, 'labels': labels, 'overflow': overflow, 'stats': {'decode_kernel': 'stand-in'}}

  def last_overflow(self, n_utt=None):
    return self.flags


_NEED = [100, 40000, 100, 300000, 100, 100, 100, 100]


def test_the_table_follows_the_overflow_retry():
  model, args = _model()
  seqs = _numbered(7)
  dec = _Regrouped(cap_need={2: 40, 5: 100})
  model._get_decoder = lambda device=None: dec  # pylint: disable=protected-access
  out = model.predict(seqs, args, min_turn=_turns(seqs))
  assert out == [[k] * s.shape[0] for k, s in enumerate(seqs)]
  assert [numbers for numbers, _, _ in dec.calls][:2] == [list(range(7)), [2, 5]] and len(dec.calls) >= 3
  assert dec.calls[-1][0] == [5]


def test_the_table_follows_the_halves_after_oom_and_the_shards():
  model, args = _model()
  seqs = _numbered(11)
  dec = _Regrouped(room=3)
  model._get_decoder = lambda device=None: dec  # pylint: disable=protected-access
  out = model.predict(seqs, args, min_turn=_turns(seqs))
  assert out == [[k] * s.shape[0] for k, s in enumerate(seqs)]
  assert dec.calls[0][0] == list(range(11)) and dec.calls[1][0] == list(range(0, 11, 2))
  dec = _Regrouped(room=3)
  out = uisrnn_amd.parallel_predict(model, seqs, args, devices=[0], min_turn=_turns(seqs))
  assert out == [[k] * s.shape[0] for k, s in enumerate(seqs)]
  # a shard of a list is a _decode_batch of its members' tables (parallel_predict's workers call exactly this)
  shard = [7, 2, 9]
  dec = _Regrouped()
  worker = types.SimpleNamespace(_model=model, _decoder=dec)
  out = host._Worker.decode(worker, [seqs[k] for k in shard], args, min_turn=[2 + k for k in shard])  # pylint: disable=protected-access
  assert out == [[k] * seqs[k].shape[0] for k in shard] and dec.calls[0][0] == shard


@pytest.mark.parametrize('room', [99, 3])
def test_the_table_follows_the_look_ahead_retry_groups(room):
  model, args = _model(look_ahead=3)
  seqs = _numbered(8, _NEED)
  dec = _Regrouped(room=room)
  model._get_decoder = lambda device=None: dec  # pylint: disable=protected-access
  out = model.predict(seqs, args, min_turn=_turns(seqs))
  assert out == [[k] * s.shape[0] for k, s in enumerate(seqs)]
  assert sorted({cap for _, cap, _ in dec.calls}) == [32768, 262144, 524287]
  # (utterance 3 needs the largest capacity: it got there, with its entry of the table -- _Regrouped checked it)
  assert any(3 in numbers and cap == 524287 for numbers, cap, _ in dec.calls)
  assert room < 99 or [1, 3] in [numbers for numbers, _, _ in dec.calls]


def test_an_int_is_every_utterances_value_and_no_rule_is_no_keyword():
  model, args = _model()
  seqs = _numbered(3)
  seen = []

  class _Plain:
    def decode_f64(self, seqs, beam_size, look_ahead, test_iteration, max_clusters=0, flags=0, level_cap=0, **tables):
      seen.append(dict(tables))
      return {'status': 0, 'labels': np.zeros(sum(s.shape[0] for s in seqs), dtype=np.int32),
              'overflow': np.zeros(len(seqs), dtype=np.int32), 'stats': {}}

  model._get_decoder = lambda device=None: _Plain()  # pylint: disable=protected-access
  model.predict(seqs, args)
  model.predict(seqs, args, min_turn=None)
  model.predict(seqs, args, min_turn=0)
  model.predict(seqs, args, min_turn=[1, 0, 1])
  model.predict(seqs, args, min_turn=3)
  model.predict_single(seqs[0], args, min_turn=4)
  assert seen == [{}, {}, {}, {}, {'min_turn': [3, 3, 3]}, {'min_turn': [4]}]


def test_the_fifth_table_on_the_host(tmp_path):
  """tests/turn_tables_main.cpp against csrc/uis_call_tables.h, built with the host compiler alone: every rule with a
  pending min_turn table, the order of the refusals, the setter, the count check."""
  cxx = shutil.which(os.environ.get('CXX', '') or 'g++') or shutil.which('c++') or shutil.which('clang++')
  if not cxx:
    pytest.skip('no host C++ compiler')
  exe = str(tmp_path / 'turn_tables')
  subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-I', os.path.join(_ROOT, 'uisrnn_amd', 'csrc'),
                  '-I', os.path.join(_ROOT, 'include'), os.path.join(_ROOT, 'tests', 'turn_tables_main.cpp'), '-o', exe], check=True)
  done = subprocess.run([exe], capture_output=True, text=True)
  assert done.returncode == 0 and done.stdout.startswith('turn_tables: ok'), (done.returncode, done.stdout, done.stderr)
