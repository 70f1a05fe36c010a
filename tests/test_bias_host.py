"""Per-frame transition_bias on the CPU: the reference the GPU tests compare with, and the surface.

tests/bias_ref.py restates the beam search with one (lp_stay, lp_sw) pair per frame on tests/limit_ref.py.  With no
table, an all-NaN table and a table that holds the model's own value it is oracle.decode bit for bit, which is what
makes it a reference.  The hard constraints are checked on the labels alone, not through the reference's own code.
Then the condition the GPU tests rest on (table P changes the labels of at least a quarter of the utterances
compared), the ValueError cases of the keyword and the new symbol.  No GPU needed.
"""

import os
import re
import types

import numpy as np
import pytest

import bias_ref
import forced_ref
import golden_util
import instantiation_cases as ic
import primed_ref
import uisrnn_amd
from uisrnn_amd import _capi
from uisrnn_amd import uisrnn as host

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _short(case, n_utt=2, frames=10):
  return [s[:frames] for s in case['seqs'][:n_utt]]


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2', 'd20_h24_depth3'])
@pytest.mark.parametrize('look_ahead', [1, 2, 3])
@pytest.mark.parametrize('test_iteration', [1, 2])
def test_without_values_of_its_own_it_is_the_oracle_decode(name, look_ahead, test_iteration, oracle_lib):
  case = golden_util.load_case(name)
  seqs = _short(case, 2, 10 if look_ahead < 3 else 7) + [case['seqs'][-1][:1]]
  beam = 4 if look_ahead < 3 else 3
  p0 = float(case['params']['transition_bias'])
  ref = oracle_lib.decode(case['params'], seqs, beam, look_ahead, test_iteration, n_threads=2)
  for what, make in (('no table', None), ('all NaN', lambda n: np.full(n, np.nan)), ('all p0', lambda n: np.full(n, p0))):
    biases = None if make is None else [make(len(s)) for s in seqs]
    got = bias_ref.decode_list(case['params'], seqs, beam, look_ahead, test_iteration, biases=biases)
    for u in range(len(seqs)):
      assert np.array_equal(got['labels'][u], ref['labels'][u]), (what, u)
    assert np.array_equal(_bits(got['scores']), _bits(ref['scores'])), what
    assert np.array_equal(_bits(got['beam_scores']), _bits(ref['beam_scores'])), what
    assert np.array_equal(got['max_clusters'], ref['max_clusters']), what


def _holds(labels, table):
  """The hard constraints, read off the labels: a 0 keeps the previous label, a 1 changes it."""
  for t in range(1, len(labels)):
    if table[t] == 0.0 and labels[t] != labels[t - 1]:
      return False
    if table[t] == 1.0 and labels[t] == labels[t - 1]:
      return False
  return True


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2', 'd20_h24_depth3'])
@pytest.mark.parametrize('look_ahead,test_iteration', [(1, 1), (1, 2), (2, 1), (3, 2)])
def test_the_hard_constraints_hold_in_every_hypothesis(name, look_ahead, test_iteration, oracle_lib):
  case = golden_util.load_case(name)
  for u, seq in enumerate(_short(case, 3, 12 if look_ahead < 3 else 8)):
    table = bias_ref.pattern(u, len(seq))
    got = bias_ref.decode(case['params'], seq, 4 if look_ahead < 3 else 3, look_ahead, test_iteration, bias=table)
    assert got['beam'], 'the pattern emptied the beam'
    n = len(seq)
    for hyp in got['beam']:
      # (every pass of test_iteration obeys it; the seam between two passes is frame 0's entry, never a 0)
      for k in range(test_iteration):
        assert _holds(hyp.trace[k * n:(k + 1) * n], table), (u, hyp.trace)


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2'])
def test_all_stay_all_change_and_a_contradiction(name, oracle_lib):
  case = golden_util.load_case(name)
  seq = case['seqs'][0][:11]
  n = len(seq)
  for look_ahead in (1, 2):
    # 0 beyond frame 0: one speaker, and the beam never widens -- at forced_ref's score of the all-zeros labeling under
    # a prior of log(1 - 0) = 0 per stay
    stay = np.zeros(n)
    stay[0] = np.nan
    got = bias_ref.decode(case['params'], seq, 5, look_ahead, 1, bias=stay)
    assert got['labels'].tolist() == [0] * n and len(got['beam']) == 1
    score, _ = bias_ref.score_one(case['params'], seq, [0] * n, stay)
    assert _bits(score) == _bits(got['score'])
    # 1 everywhere under limit 2: the two speakers alternate
    got = bias_ref.decode(case['params'], seq, 5, look_ahead, 1, limit=2, bias=np.ones(n))
    assert got['labels'].tolist() == [t % 2 for t in range(n)]
  # 1 under limit 1: frame 1 can neither stay nor open a cluster
  got = bias_ref.decode(case['params'], seq, 5, 1, 1, limit=1, bias=np.ones(n))
  assert not got['beam'] and got['labels'].tolist() == [-1] * n and np.isposinf(got['score'])
  # 0 at frame 0: no hypothesis has a previous label (what _check_transition_bias refuses)
  got = bias_ref.decode(case['params'], seq, 5, 1, 1, bias=np.zeros(n))
  assert not got['beam']


def test_score_one_and_the_session_agree_with_the_decode(oracle_lib):
  case = golden_util.load_case('tiny_d16')
  seq = case['seqs'][0][:20]
  table = bias_ref.pattern(2, len(seq))
  offline = bias_ref.decode(case['params'], seq, 4, 1, 1, bias=table)
  score, losses = bias_ref.score_one(case['params'], seq, offline['labels'], table)
  assert _bits(score) == _bits(offline['score']) and np.isfinite(losses).all()
  # without a table score_one is forced_ref's
  want, want_losses = forced_ref.score_one(case['params'], seq, offline['labels'])
  got, got_losses = bias_ref.score_one(case['params'], seq, offline['labels'])
  assert _bits(got) == _bits(want) and np.array_equal(_bits(got_losses), _bits(want_losses))
  session = bias_ref.Session(case['params'], 4)
  for t0 in range(0, len(seq), 6):
    session.push(seq[t0:t0 + 6], table[t0:t0 + 6])
  assert session.labels() == offline['labels'].tolist()
  assert np.array_equal(_bits(session.scores()), _bits([h.score for h in offline['beam']]))


def changed_share(pairs):
  """pairs: (unbiased labels, biased labels) of the utterances a test compares.  Among those of at least three frames
  the share whose labels table P changes; raises where it is below a quarter: such a test would pass vacuously."""
  long_ones = [(a, b) for a, b in pairs if len(a) >= 3]
  changed = sum(not np.array_equal(a, b) for a, b in long_ones)
  if not long_ones or 4 * changed < len(long_ones):
    raise RuntimeError('table P changes {} of {} utterances: the comparison would be vacuous'.format(changed, len(long_ones)))
  return changed, len(long_ones)


@pytest.mark.parametrize('row', [r for r in ic.ROWS if r[0] == ic.RESIDENT and r[1:] in ((128, 128, 0, 0), (256, 128, 0, 0))],
                         ids=ic.row_id)
def test_the_pattern_changes_the_labels_of_a_quarter(row, oracle_lib):
  pairs = []
  for case in ic.CASES[row]:
    model = primed_ref.Model(case.params())
    seqs = case.utterances(8)
    free = oracle_lib.decode(case.params(), seqs, case.beam, case.look_ahead, case.test_iteration, n_threads=4)
    for u in range(0, len(seqs), 2):
      got = bias_ref.decode(model, seqs[u], case.beam, case.look_ahead, case.test_iteration,
                            bias=bias_ref.pattern(u, len(seqs[u])))
      assert got['beam'], (case.name, u)
      assert _holds(got['labels'], bias_ref.pattern(u, len(seqs[u]))), (case.name, u)
      pairs.append((free['labels'][u], got['labels']))
  changed_share(pairs)
  with pytest.raises(RuntimeError):
    changed_share([(a, a) for a, _ in pairs])


# ---- the surface

def test_the_new_symbol_is_declared_bound_and_exported():
  header = open(os.path.join(_ROOT, 'include', 'uisrnn_hip.h')).read()
  assert re.search(r'int32_t uis_frame_bias\(uis_handle\* h, const double\* bias, int64_t n_frames\);', header)
  assert 'uis_frame_bias' in _capi.EXPORTED_SYMBOLS
  assert re.search(r'#define UIS_ABI_VERSION 6\b', header) and _capi.UIS_ABI_VERSION == 6
  lib = _capi.load_library()
  assert lib.uis_abi_version() == 6
  assert lib.uis_frame_bias.argtypes is not None
  assert lib.uis_frame_bias(None, None, 0) == _capi.UIS_ERR_INVALID_ARG   # a null handle is refused, not dereferenced
  for fn in ('predict', 'predict_single', 'predict_nbest', 'predict_posteriors', 'score_labels', 'score_speakers'):
    assert 'transition_bias' in getattr(uisrnn_amd.UISRNN, fn).__code__.co_varnames, fn
  assert 'transition_bias' not in uisrnn_amd.UISRNN.predict_primed.__code__.co_varnames
  assert 'transition_bias' in host.parallel_predict.__code__.co_varnames
  assert 'transition_bias' in host.OnlineSession.push.__code__.co_varnames
  assert 'transition_bias' in host.StreamPool.push.__code__.co_varnames


def test_the_keyword_as_the_librarys_table():
  check = host._check_transition_bias  # pylint: disable=protected-access
  nan = float('nan')
  assert check(None, [3, 2]) is None
  got = check(0.25, [3, 0, 2])
  assert [g.tolist() for g in got] == [[0.25] * 3, [], [0.25] * 2] and all(g.dtype == np.float64 for g in got)
  got = check([[nan, 0, 1], None], [3, 2])
  assert np.isnan(got[0][0]) and got[0][1:].tolist() == [0.0, 1.0] and np.isnan(got[1]).all()
  assert check(np.array([0.5, 0.0]), [2], single=True)[0].tolist() == [0.5, 0.0]
  assert check([np.array([0.5, 0.0])], [2], single=True)[0].tolist() == [0.5, 0.0]
  assert check(np.array(1), [2])[0].tolist() == [1.0, 1.0]   # a 0-d array is a scalar
  assert check(1, [2])[0].tolist() == [1.0, 1.0]
  # a session's chunk may begin with a 0; an offline decode may not
  assert check([[0.0, 0.5]], [2], offline=False)[0].tolist() == [0.0, 0.5]
  assert check(0.0, [0]) is not None   # (no frame, nothing to contradict)
  for bad in (True, np.bool_(False), 'often', 1.5, -0.1, float('inf'), -float('inf'), 0, 0.0,
              [[0.5, 0.5, 0.5]], [[0.5, 0.5], [0.5, 0.5]], [[0.5, 0.5, 0.5], [2.0, 0.5]], [[0.5, 0.5, 0.5], [0.5, float('inf')]],
              [[0.5, 0.5, 0.5], [0.0, 0.5]], [[0.5, True, 0.5], [0.5, 0.5]], [np.array([True, False, True]), None],
              np.array([0.5, 0.5, 0.5, 0.5, 0.5]), [[0.5, 0.5, 0.5], [[0.5, 0.5]]]):
    with pytest.raises(ValueError):
      check(bad, [3, 2])


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
  ids = [[0, 0, 1], [0, 1]]
  for bad in (True, 1.5, float('inf'), 0.0, [[0.5, 0.5, 0.5]], [[0.5, 0.5], [0.5, 0.5]], [[0.0, 0.5, 0.5], [0.5, 0.5]]):
    for call in (lambda b: model.predict(seqs, args, transition_bias=b),
                 lambda b: model.predict_nbest(seqs, args, transition_bias=b),
                 lambda b: model.predict_posteriors(seqs, args, transition_bias=b),
                 lambda b: host.parallel_predict(model, seqs, args, transition_bias=b)):
      with pytest.raises(ValueError):
        call(bad)
  for bad in (True, 1.5, [[0.5, 0.5, 0.5]], [[0.5, 0.5], [0.5, 0.5]]):
    for call in (lambda b: model.score_labels(seqs, ids, transition_bias=b),
                 lambda b: model.score_speakers(seqs, ids, transition_bias=b)):
      with pytest.raises(ValueError):
        call(bad)
  for bad in (True, 1.5, -1, [0.5, 0.5], [0.0, 0.5, 0.5], [[0.5, 0.5, 0.5], [0.5, 0.5, 0.5]]):
    with pytest.raises(ValueError):
      model.predict_single(seqs[0], args, transition_bias=bad)
    with pytest.raises(ValueError):
      model.predict(seqs[0], args, transition_bias=bad)
