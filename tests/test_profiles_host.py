"""Speaker profiles without a GPU: the CPU restatement (tests/profiles_ref.py) against a float64 computation and
against speakers_ref's means, closed cases, sigma2_estimate and speaker_distances on hand-made profiles, the symbol
surface and the argument checks that precede any device work.

test_the_restatement_against_float64 and test_closed_cases check tests/profiles_ref.py itself -- the yardstick the GPU
tests compare the library with -- and touch nothing of the library, so they pass on a tree without the entry points;
every other test here, and every test of tests/test_gpu_profiles.py, fails there."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import golden_util
import profiles_ref
import speakers_ref
import uisrnn_amd
from oracle import oracle
from uisrnn_amd import _capi, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -23


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _params(model):
  if model.startswith('trained_'):
    return weights.load_checkpoint(os.path.join(golden_util.GOLDEN_DIR, model + '.uisrnn'))
  return golden_util.load_case(model)['params']


def _normal(seed, n, dim):
  return np.random.default_rng(seed).standard_normal((n, dim))


def _final_means(params, seq, labels, monkeypatch):
  """The means speakers_ref.rows_one carries after the last frame: one more frame is appended and the means it is
  scored against are recorded (rows_one hands every open cluster's mean to oracle.weighted_mse)."""
  seen = []
  real = oracle.weighted_mse

  def recording(mse_params, mean, x):
    seen.append((np.array(x, dtype=np.float32), np.array(mean, dtype=np.float32)))
    return real(mse_params, mean, x)

  extra = np.full((1, seq.shape[1]), 0.25)
  monkeypatch.setattr(speakers_ref.oracle, 'weighted_mse', recording)
  speakers_ref.rows_one(params, np.concatenate([seq, extra]), np.concatenate([labels, [0]]).astype(np.int32))
  monkeypatch.undo()
  count = speakers_ref.cluster_count(labels)
  last = [mean for x, mean in seen if np.array_equal(x, extra[0].astype(np.float32))]
  assert len(last) == count + 1   # every open cluster, then m0
  return np.stack(last[:count])


@pytest.mark.parametrize('model,n', [('tiny_d16', 48), ('trained_d256', 32)])
def test_the_restatement_against_float64(model, n, oracle_lib, monkeypatch):
  """sum_r2 and sum_x within the rounding of their own operations of a float64 computation on the same float32
  observations and the restatement's own float32 mean rows; the means are speakers_ref's, bit for bit.

  sum_r2: one rounding in the difference, two in the square as formed, n - 1 in the sum of non-negative terms -- first
  order (n + 2) 2^-24 relative, a factor 2 of margin.  sum_x: n 2^-23 of sum |x|.  N(0, 1) observations: no product
  underflows."""
  del oracle_lib
  params = _params(model)
  dim = int(params['observation_dim'])
  seq = _normal(9900, n, dim)
  labels = speakers_ref.revisiting(n, clusters=6)
  prof = profiles_ref.profile_one(params, seq, labels, want_score=False)
  x = seq.astype(np.float32)
  assert prof.n_clusters == 6
  for k in range(6):
    at = np.flatnonzero(labels == k)
    x64, p64 = x[at].astype(np.float64), prof.priors[at].astype(np.float64)
    ref_r2 = ((x64 - p64) ** 2).sum(axis=0)
    ref_x = x64.sum(axis=0)
    assert np.all(ref_r2 > 1e-30)
    assert np.all(np.abs(prof.sum_r2[k].astype(np.float64) - ref_r2) <= (len(at) + 2) * EPS * ref_r2), k
    assert np.all(np.abs(prof.sum_x[k].astype(np.float64) - ref_x) <= len(at) * EPS * np.abs(x64).sum(axis=0)), k
  assert np.array_equal(_bits(prof.mean), _bits(_final_means(params, seq, labels, monkeypatch)))
  assert np.array_equal(prof.stats, profiles_ref.stats_numpy(labels))


def test_closed_cases(oracle_lib):
  del oracle_lib
  params = _params('tiny_d16')
  m0, _ = oracle.constants(params)
  seq = _normal(9910, 40, 16)
  x = seq.astype(np.float32)
  # every cluster has one frame
  prof = profiles_ref.profile_one(params, seq[:12], speakers_ref.all_new(12), want_score=False)
  assert prof.n_clusters == 12 and prof.stats.tolist() == [[1, 1, t, t] for t in range(12)]
  assert np.array_equal(_bits(prof.sum_x), _bits(x[:12]))
  d = (x[:12] - m0).astype(np.float32)
  assert np.array_equal(_bits(prof.sum_r2), _bits((d * d).astype(np.float32)))
  # one cluster over the whole utterance
  prof = profiles_ref.profile_one(params, seq, speakers_ref.one_cluster(40), want_score=False)
  assert prof.n_clusters == 1 and prof.stats.tolist() == [[40, 1, 0, 39]]
  # the hand-made labelings of speakers_ref
  prof = profiles_ref.profile_one(params, seq, speakers_ref.revisiting(40), want_score=False)
  assert prof.n_clusters == 18 and np.array_equal(prof.stats, profiles_ref.stats_numpy(speakers_ref.revisiting(40)))
  assert prof.stats[:, 0].sum() == 40 and np.all(prof.stats[:, 2] == 2 * np.arange(18))
  prof = profiles_ref.profile_one(params, seq, speakers_ref.invalid_at(40))
  assert prof.n_clusters == -1 and prof.mean.shape == (0, 16) and np.isposinf(prof.score)
  pad = profiles_ref.padded([prof], 3, 16)
  assert pad['n_clusters'].tolist() == [-1] and np.all(pad['stats'] == [0, 0, -1, -1])
  assert not any(_bits(pad[key]).any() for key in ('mean', 'sum_x', 'sum_r2'))
  empty = profiles_ref.profile_one(params, seq[:0], np.zeros(0, np.int32))
  assert empty.n_clusters == 0 and empty.score == 0.0


def _model(**over):
  model_args, _, _ = uisrnn_amd.parse_arguments([])
  model_args.observation_dim = 4
  model_args.rnn_hidden_size = 8
  model_args.transition_bias = 0.2
  model_args.sigma2 = 0.05
  for key, val in over.items():
    setattr(model_args, key, val)
  return uisrnn_amd.UISRNN(model_args)


def _hand_made(ids, frames, mean, sum_r2):
  k = len(ids)
  z = np.zeros(k, dtype=np.int32)
  return uisrnn_amd.SpeakerProfile(ids, np.array(frames, dtype=np.int32), z + 1, z, z, np.array(mean, dtype=np.float32),
                                   np.zeros((k, 4), np.float32), np.array(sum_r2, dtype=np.float32), 0.0)


def test_sigma2_estimate_and_speaker_distances_on_hand_made_profiles(monkeypatch):
  model = _model()
  a = _hand_made(['x', 'y'], [3, 1], [[0, 0, 0, 0], [1, 2, 3, 4]], [[1, 2, 3, 4], [0.5, 0.5, 0.5, 0.5]])
  b = _hand_made([7], [4], [[1, 0, 0, 0]], [[2, 2, 2, 2]])
  monkeypatch.setattr(model, 'speaker_profiles', lambda seqs, ids: [a, b])
  before = np.array(model.sigma2, copy=True)
  got = model.sigma2_estimate(['ignored'], ['ignored'])
  assert got.dtype == np.float64 and got.tolist() == [3.5 / 8, 4.5 / 8, 5.5 / 8, 6.5 / 8]
  assert np.array_equal(model.sigma2, before)   # nothing of the model changes
  assert isinstance(model.estimate_sigma2, bool)   # (the reference's training flag keeps its name)
  monkeypatch.setattr(model, 'speaker_profiles', lambda seqs, ids: a)   # a single sequence
  assert model.sigma2_estimate('ignored', 'ignored').tolist() == [1.5 / 4, 2.5 / 4, 3.5 / 4, 4.5 / 4]
  assert a.centroid.dtype == np.float64 and a.centroid.shape == (2, 4)
  # sigma2 0.05: weight 10 per dimension
  dist = uisrnn_amd.speaker_distances(model, a, b)
  assert dist.dtype == np.float64 and dist.shape == (2, 1)
  assert np.allclose(dist[:, 0], [10.0 * 1, 10.0 * (0 + 4 + 9 + 16)], rtol=1e-6)   # (sigma2 is float32)
  model.sigma2 = np.array([0.5, 1.0, 2.0, 4.0])
  dist = uisrnn_amd.speaker_distances(model, a.mean, {'mean': b.mean})   # arrays and session profiles
  assert dist[1, 0] == 0.0 / 1 + 4.0 / 2 + 9.0 / 4 + 16.0 / 8
  assert uisrnn_amd.speaker_distances(model, np.zeros((0, 4)), b).shape == (0, 1)
  for bad in (np.zeros(4), np.zeros((2, 3)), {'mean': np.zeros((2, 5))}):
    with pytest.raises(ValueError, match='observation_dim'):
      uisrnn_amd.speaker_distances(model, a, bad)


def test_symbol_surface():
  header = open(os.path.join(ROOT, 'include', 'uisrnn_hip.h')).read()
  lib = _capi.load_library()
  exported = subprocess.check_output(['nm', '-D', '--defined-only', lib._name]).decode()  # pylint: disable=protected-access
  for name in ('uis_speaker_profiles', 'uis_session_profiles'):
    assert re.search(r'^int32_t\s+' + name + r'\s*\(', header, re.M)
    assert name in _capi.EXPORTED_SYMBOLS and getattr(lib, name).argtypes
    assert re.search(r'\bT ' + name + '$', exported, re.M)
  assert lib.uis_abi_version() == 6 and _capi.UIS_ABI_VERSION == 6
  assert callable(_capi.Decoder.speaker_profiles) and callable(_capi.Decoder.stream_profiles)
  for name in ('speaker_profiles', 'sigma2_estimate'):
    assert callable(getattr(uisrnn_amd.UISRNN, name))
  assert callable(uisrnn_amd.OnlineSession.profiles) and callable(uisrnn_amd.StreamPool.profiles)
  assert uisrnn_amd.speaker_distances is uisrnn_amd.uisrnn.speaker_distances


def test_c_abi_rejects_bad_arguments_without_a_device():
  """What can be refused without a handle is: a null handle.  (The width, length and null-pointer checks behind a
  handle run before any device work, but a handle needs a device: tests/test_gpu_profiles.py.)"""
  lib = _capi.load_library()
  off = np.array([0, 2], dtype=np.int64)
  lab = np.array([0, 1], dtype=np.int32)
  n, stats, mean = np.zeros(1, np.int32), np.zeros(8, np.int32), np.zeros(8, np.float32)
  i32p, fp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
  rc = lib.uis_speaker_profiles(None, None, off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1, lab.ctypes.data_as(i32p), 2,
                                n.ctypes.data_as(i32p), stats.ctypes.data_as(i32p), mean.ctypes.data_as(fp), None, None, None)
  assert rc == _capi.UIS_ERR_INVALID_ARG
  rc = lib.uis_session_profiles(None, 2, n.ctypes.data_as(i32p), stats.ctypes.data_as(i32p), mean.ctypes.data_as(fp))
  assert rc == _capi.UIS_ERR_INVALID_ARG
  assert not n.any() and not stats.any() and not mean.any()


def test_python_argument_errors_before_any_device(monkeypatch):
  """score_labels' refusals, raised before a decoder handle is created."""
  def no_device(*args, **kwargs):
    raise AssertionError('a device handle was requested')
  monkeypatch.setattr(_capi, 'Decoder', no_device)
  model = _model(observation_dim=16)
  seq = np.zeros((4, 16))
  for call in (model.speaker_profiles, model.sigma2_estimate):
    with pytest.raises(TypeError, match='test_sequence should be a numpy array of float type.'):
      call(np.zeros((4, 16), dtype=np.float32), [0] * 4)
    with pytest.raises(ValueError, match='test_sequence must be 2-dim array.'):
      call(np.zeros(16), [0])
    with pytest.raises(ValueError, match='does not match the dimension specified by args.observation_dim'):
      call(np.zeros((4, 15)), [0] * 4)
    with pytest.raises(TypeError, match='test_sequences should be either a list or numpy array.'):
      call('abc', [0])
    with pytest.raises(ValueError):
      call(seq, [0] * 3)
    with pytest.raises(ValueError):
      call([seq, seq], [[0] * 4])
  with pytest.raises(TypeError, match='transition_bias is None'):
    _model(observation_dim=16, transition_bias=None).speaker_profiles(seq, [0] * 4)
