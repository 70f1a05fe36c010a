"""max_speakers on the CPU: the reference the GPU tests compare with, and the surface.

tests/limit_ref.py restates the beam search with a per-utterance bound, test_iteration and any look_ahead from the
oracle's CoreRNN row and weighted MSE.  With no limit it is oracle.decode bit for bit -- labels, scores, the final
beam, the largest cluster count -- which is what makes it a reference.  With a limit: no trace names more clusters
than it, limit 1 is the all-zeros labeling at forced_ref's score, a limit the unbounded decode never reaches changes
nothing.  Then the new symbols (declared, bound, exported; the ABI version stays 6) and the ValueError cases of the
max_speakers keyword.  No GPU needed.
"""

import os
import re
import types

import numpy as np
import pytest

import forced_ref
import golden_util
import limit_ref
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
def test_without_a_limit_it_is_the_oracle_decode(name, look_ahead, test_iteration, oracle_lib):
  case = golden_util.load_case(name)
  # (look_ahead 3 enumerates beam * K^3 tuples per window in Python: short utterances, one of a ragged last window)
  seqs = _short(case, 2, 10 if look_ahead < 3 else 7) + [case['seqs'][-1][:1]]
  beam = 4 if look_ahead < 3 else 3
  ref = oracle_lib.decode(case['params'], seqs, beam, look_ahead, test_iteration, n_threads=2)
  got = limit_ref.decode_list(case['params'], seqs, beam, look_ahead, test_iteration)
  for u in range(len(seqs)):
    assert np.array_equal(got['labels'][u], ref['labels'][u]), u
  assert np.array_equal(_bits(got['scores']), _bits(ref['scores']))
  assert np.array_equal(_bits(got['beam_scores']), _bits(ref['beam_scores']))
  assert np.array_equal(got['max_clusters'], ref['max_clusters'])
  # limits of 0 / None are no limits
  again = limit_ref.decode_list(case['params'], seqs[:1], beam, look_ahead, test_iteration, limits=[0])
  assert np.array_equal(_bits(again['beam_scores']), _bits(ref['beam_scores'][:1]))


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2'])
@pytest.mark.parametrize('look_ahead,test_iteration', [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_no_trace_names_more_clusters_than_its_limit(name, look_ahead, test_iteration, oracle_lib):
  case = golden_util.load_case(name)
  seqs = _short(case, 2, 12)
  free = oracle_lib.decode(case['params'], seqs, 4, look_ahead, test_iteration, n_threads=2)
  for u, seq in enumerate(seqs):
    for limit in (1, 2, 3):
      got = limit_ref.decode(case['params'], seq, 4, look_ahead, test_iteration, limit)
      assert got['max_clusters'] <= limit
      for hyp in got['beam']:
        assert len(hyp.means) <= limit and max(hyp.trace) < limit, (u, limit)
      assert np.isfinite(got['score'])
    # a limit the unbounded decode never reaches changes nothing
    k_free = int(free['max_clusters'][u])
    for limit in (k_free, k_free + 1, 4096):
      got = limit_ref.decode(case['params'], seq, 4, look_ahead, test_iteration, limit)
      assert np.array_equal(got['labels'], free['labels'][u]), (u, limit)
      assert np.array_equal(_bits(got['beam_scores']), _bits(free['beam_scores'][u])), (u, limit)


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2', 'd20_h24_depth3'])
def test_limit_1_is_one_speaker_at_the_forced_score(name, oracle_lib):
  case = golden_util.load_case(name)
  seqs = _short(case, 3, 14)
  zeros = [np.zeros(len(s), dtype=np.int32) for s in seqs]
  want, _ = forced_ref.score(case['params'], seqs, zeros)
  for look_ahead in (1, 2):
    got = limit_ref.decode_list(case['params'], seqs, 5, look_ahead, 1, limits=[1] * len(seqs))
    for u in range(len(seqs)):
      assert not got['labels'][u].any()
      assert len(got['outs'][u]['beam']) == 1   # one candidate per step: the beam never widens
    assert np.array_equal(_bits(got['scores']), _bits(want))


def test_a_session_whose_limit_changes(oracle_lib):
  case = golden_util.load_case('tiny_d16')
  seq = case['seqs'][0]
  # a constant limit: the offline bounded decode, whatever the chunking
  offline = limit_ref.decode(case['params'], seq, 4, 1, 1, limit=2)
  session = limit_ref.Session(case['params'], 4, limit=2)
  for t0 in range(0, len(seq), 5):
    session.push(seq[t0:t0 + 5])
  assert session.labels() == offline['labels'].tolist()
  assert np.array_equal(_bits(session.scores()), _bits([h.score for h in offline['beam']]))
  # raised 1 -> 3 after eight frames: one speaker until then, at most three afterwards; lowered to 1 while K is
  # above it: the hypotheses stay and open nothing more
  session = limit_ref.Session(case['params'], 4, limit=1)
  session.push(seq[:8])
  assert session.K() == 1
  session.set_limit(3)
  session.push(seq[8:16])
  k_mid = session.K()
  assert 1 < k_mid <= 3
  session.set_limit(1)
  session.push(seq[16:])
  assert session.K() == k_mid and max(session.labels()) < k_mid


# ---- the surface

def test_the_new_symbols_are_declared_bound_and_exported():
  header = open(os.path.join(_ROOT, 'include', 'uisrnn_hip.h')).read()
  for name, args in (('uis_decode_limits', r'uis_handle\* h, const int32_t\* limits, int32_t n_utt'),
                     ('uis_stream_limits', r'uis_handle\* h, const int32_t\* limits'),
                     ('uis_stream_get_limits', r'uis_handle\* h, int32_t\* out')):
    assert re.search(r'int32_t %s\(%s\);' % (name, args), header), name
    assert name in _capi.EXPORTED_SYMBOLS
  assert re.search(r'#define UIS_ABI_VERSION 6\b', header) and _capi.UIS_ABI_VERSION == 6
  lib = _capi.load_library()
  assert lib.uis_abi_version() == 6
  for name in ('uis_decode_limits', 'uis_stream_limits', 'uis_stream_get_limits'):
    assert getattr(lib, name).argtypes is not None
  # null handles are refused, not dereferenced
  assert lib.uis_decode_limits(None, None, 0) == _capi.UIS_ERR_INVALID_ARG
  assert lib.uis_stream_limits(None, None) == _capi.UIS_ERR_INVALID_ARG
  assert lib.uis_stream_get_limits(None, None) == _capi.UIS_ERR_INVALID_ARG
  for fn in ('predict', 'predict_single', 'predict_nbest', 'predict_posteriors', 'predict_primed', 'online',
             'online_pool'):
    assert 'max_speakers' in getattr(uisrnn_amd.UISRNN, fn).__code__.co_varnames, fn
  assert 'max_speakers' in host.parallel_predict.__code__.co_varnames
  assert 'max_speakers' in host.StreamPool.open.__code__.co_varnames
  assert callable(host.OnlineSession.set_max_speakers) and callable(host.OnlineSession.max_speakers)


def test_the_keyword_as_the_librarys_table():
  args = types.SimpleNamespace()
  check = host._check_max_speakers  # pylint: disable=protected-access
  assert check(None, args, 3) is None
  assert check(0, args, 3) is None and check([None, 0, None], args, 3) is None
  assert check(2, args, 3) == [2, 2, 2]
  assert check(2.0, args, 2) == [2, 2]
  assert check(np.int64(5), args, 1) == [5]
  assert check([3, None, 0, 4096], args, 4) == [3, 0, 0, 4096]
  assert check(np.array([1, 2]), args, 2) == [1, 2]
  assert check(np.array(3), args, 2) == [3, 3]    # a 0-d array is a scalar
  # rides on the args object, the way max_clusters does; the keyword wins
  assert check(None, types.SimpleNamespace(max_speakers=4), 2) == [4, 4]
  assert check(2, types.SimpleNamespace(max_speakers=4), 2) == [2, 2]
  for bad in (True, False, 2.5, -1, 4097, float('nan'), 'two', [1, 2], [1, 2, 3, 4], [1, True, 2], [1, -2, 3],
              [1, 2.5, 3], np.array([1.5, 2, 3]), np.array(2.5), np.array([[1, 2, 3]])):
    with pytest.raises(ValueError):
      check(bad, args, 3)


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
  for bad in (True, 1.5, -1, 4097, [1], [1, 2, 3]):
    for call in (lambda b: model.predict(seqs, args, max_speakers=b),
                 lambda b: model.predict_nbest(seqs, args, max_speakers=b),
                 lambda b: model.predict_posteriors(seqs, args, max_speakers=b),
                 lambda b: model.predict_primed(seqs, [[0], [0]], args, max_speakers=b),
                 lambda b: host.parallel_predict(model, seqs, args, max_speakers=b),
                 lambda b: model.online(2, args, 16, max_speakers=b),
                 lambda b: model.online_pool(2, args, 16, max_speakers=b)):
      with pytest.raises(ValueError):
        call(bad)
  for bad in (True, 1.5, -1, 4097, [1, 2]):
    with pytest.raises(ValueError):
      model.predict_single(seqs[0], args, max_speakers=bad)


def test_the_initial_cap_under_a_bound():
  cap = host._initial_cluster_cap  # pylint: disable=protected-access
  ns = types.SimpleNamespace
  # today's rule already fits: nothing changes, so the compile-time shape classes are still picked
  assert cap(ns(beam_size=10, look_ahead=1), [4, 4]) == cap(ns(beam_size=10, look_ahead=1)) == 16
  assert cap(ns(beam_size=20, look_ahead=1), [4]) == cap(ns(beam_size=20, look_ahead=1)) == 11
  # a beam so wide that the rule leaves the fast select, every utterance bounded, beam * (L + 1) <= 256: cap L
  assert cap(ns(beam_size=50, look_ahead=1)) == 16
  assert cap(ns(beam_size=50, look_ahead=1), [4, 3]) == 4
  assert cap(ns(beam_size=50, look_ahead=1), [4, 0]) == 16      # one utterance unbounded
  assert cap(ns(beam_size=50, look_ahead=1), [5]) == 16         # 50 * 6 > 256
  assert cap(ns(beam_size=50, look_ahead=1, max_clusters=9), [4]) == 9   # an explicit cap is the caller's
  assert cap(ns(beam_size=50, look_ahead=2), [4]) == 16         # the fast select is look_ahead 1's
