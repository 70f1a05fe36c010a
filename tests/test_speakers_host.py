"""score_speakers without a GPU: the CPU restatement (tests/speakers_ref.py) against the oracle's candidate scores and
against forced_ref, the symbol surface, the argument checks and speaker_posteriors."""

import os
import re
import subprocess

import numpy as np
import pytest

import forced_ref
import golden_util
import speakers_ref
import uisrnn_amd
from uisrnn_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _case(name):
  case = golden_util.load_case(name)
  return case['params'], [np.asarray(s)[:40] for s in case['seqs'][:2]]


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2', 'd20_h24_depth3', 'tracker_d64_h300'])
def test_rows_are_the_oracle_candidate_scores(name, oracle_lib):
  """Identity 2: along the labels of a beam 1, look_ahead 1, test_iteration 1 decode, float32(cum + rows) IS the
  decode's candidate array, +inf pattern included, and the running sum is the decode's score."""
  params, seqs = _case(name)
  ref = oracle_lib.decode(params, seqs, 1, 1, 1)
  for u, seq in enumerate(seqs):
    labels = ref['labels'][u]
    score, rows = speakers_ref.rows_one(params, seq, labels)
    width = rows.shape[1]
    assert width == int(labels.max()) + 2
    want = oracle_lib.candidate_scores(params, seq, 1, 1, 1, width)[:, 0]
    got = speakers_ref.candidates(rows, labels)
    assert want.shape == got.shape
    assert np.array_equal(_bits(got), _bits(want)), (name, u)
    assert _bits(score) == _bits(ref['scores'][u])


def _hand_made(n):
  return {'revisiting': speakers_ref.revisiting(n), 'one_cluster': speakers_ref.one_cluster(n),
          'all_new': speakers_ref.all_new(12), 'invalid': speakers_ref.invalid_at(n),
          'empty': np.zeros(0, np.int32), 'one_frame': np.zeros(1, np.int32)}


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2'])
def test_chosen_column_is_forced_ref(name, oracle_lib):
  """Identity 1 on the CPU side: rows[t, c_t] equals forced_ref.score_one's loss of frame t, and the totals agree."""
  del oracle_lib
  params, seqs = _case(name)
  seq = seqs[0]
  for what, labels in _hand_made(seq.shape[0]).items():
    sub = seq[:labels.shape[0]]
    want_score, want = forced_ref.score_one(params, sub, labels)
    score, rows = speakers_ref.rows_one(params, sub, labels)
    assert rows.shape == (labels.shape[0], speakers_ref.cluster_count(labels) + 1), what
    nv = int(np.isfinite(want).sum()) if what == 'invalid' else labels.shape[0]
    chosen = np.array([rows[t, labels[t]] for t in range(nv)], dtype=np.float32)
    assert np.array_equal(_bits(chosen), _bits(want[:nv])), what
    assert np.all(np.isposinf(rows[nv:])), what
    assert _bits(score) == _bits(want_score), what
    for t in range(nv):  # the padding: finite up to the new-speaker column, +inf past it
      k_t = speakers_ref.cluster_count(labels[:t])
      assert np.all(np.isfinite(rows[t, :k_t + 1])) and np.all(np.isposinf(rows[t, k_t + 1:])), (what, t)
  assert speakers_ref.cluster_count(speakers_ref.revisiting(40)) == 18
  assert speakers_ref.invalid_at(40)[20] == 4


def test_symbol_surface():
  header = open(os.path.join(ROOT, 'include', 'uisrnn_hip.h')).read()
  assert re.search(r'^int32_t\s+uis_score_speakers\s*\(', header, re.M)
  assert 'uis_score_speakers' in _capi.EXPORTED_SYMBOLS
  lib = _capi.load_library()
  exported = subprocess.check_output(['nm', '-D', '--defined-only', lib._name]).decode()  # pylint: disable=protected-access
  assert re.search(r'\bT uis_score_speakers$', exported, re.M)
  assert lib.uis_abi_version() == 6
  assert callable(_capi.Decoder.score_speakers) and callable(uisrnn_amd.UISRNN.score_speakers)
  assert uisrnn_amd.speaker_posteriors is uisrnn_amd.uisrnn.speaker_posteriors


def _model(**over):
  model_args, _, _ = uisrnn_amd.parse_arguments([])
  model_args.observation_dim = 16
  model_args.rnn_hidden_size = 8
  model_args.transition_bias = 0.2
  model_args.sigma2 = 0.05
  for key, val in over.items():
    setattr(model_args, key, val)
  return uisrnn_amd.UISRNN(model_args)


def test_score_speakers_argument_errors_before_any_device(monkeypatch):
  """score_labels' refusals, raised before a decoder handle is created."""
  def no_device(*args, **kwargs):
    raise AssertionError('a device handle was requested')
  monkeypatch.setattr(_capi, 'Decoder', no_device)
  model = _model()
  seq = np.zeros((4, 16))
  with pytest.raises(TypeError, match='test_sequence should be a numpy array of float type.'):
    model.score_speakers(np.zeros((4, 16), dtype=np.float32), [0] * 4)
  with pytest.raises(ValueError, match='test_sequence must be 2-dim array.'):
    model.score_speakers(np.zeros(16), [0])
  with pytest.raises(ValueError, match='does not match the dimension specified by args.observation_dim'):
    model.score_speakers(np.zeros((4, 15)), [0] * 4)
  with pytest.raises(TypeError, match='test_sequences should be either a list or numpy array.'):
    model.score_speakers('abc', [0])
  with pytest.raises(ValueError):
    model.score_speakers(seq, [0] * 3)
  with pytest.raises(ValueError):
    model.score_speakers([seq, seq], [[0] * 4])
  with pytest.raises(ValueError):
    model.score_speakers([seq, np.zeros((2, 3))], [[0] * 4, [0] * 2])
  with pytest.raises(TypeError, match='test_sequence should be a numpy array of float type.'):
    model.score_speakers([[[1.0] * 16]], [[0]])
  with pytest.raises(TypeError, match='transition_bias is None'):
    _model(transition_bias=None).score_speakers(seq, [0] * 4)


def test_c_abi_rejects_bad_arguments_without_a_device():
  import ctypes  # pylint: disable=import-outside-toplevel
  lib = _capi.load_library()
  off = np.array([0, 2], dtype=np.int64)
  lab = np.array([0, -1], dtype=np.int32)
  out = np.zeros(4, dtype=np.float32)
  rc = lib.uis_score_speakers(None, None, off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1,
                              lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 2,
                              out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), None)
  assert rc == _capi.UIS_ERR_INVALID_ARG


def test_speaker_posteriors():
  inf = np.inf
  losses = np.array([[1.0, 1.0 + np.log(3.0), inf],
                     [0.0, inf, inf],
                     [2.0, 2.0, 2.0],
                     [inf, inf, inf]], dtype=np.float32)
  got = uisrnn_amd.speaker_posteriors(losses)
  assert got.dtype == np.float64 and got.shape == (4, 3)
  # row 0: weights 1 and 1/3 -> 3/4, 1/4 (the float32 rounding of 1 + log 3 is all that separates them)
  assert np.allclose(got[0], [0.75, 0.25, 0.0], rtol=0, atol=1e-7) and got[0, 2] == 0.0
  assert got[1].tolist() == [1.0, 0.0, 0.0]
  assert np.allclose(got[2], [1 / 3, 1 / 3, 1 / 3], rtol=0, atol=1e-15)
  assert np.all(np.isnan(got[3]))
  # temperature 2: exp(-log(3) / 2) = 1 / sqrt 3
  hot = uisrnn_amd.speaker_posteriors(losses[:1], temperature=2.0)
  r = 1.0 / np.sqrt(3.0)
  assert np.allclose(hot[0], [1 / (1 + r), r / (1 + r), 0.0], rtol=0, atol=1e-7)
  # large losses do not underflow the row: the softmax is shifted by the row's minimum loss
  big = uisrnn_amd.speaker_posteriors(np.array([[5000.0, 5000.0]], dtype=np.float32))
  assert big[0].tolist() == [0.5, 0.5]
  for bad in (0, -1.0, np.inf, np.nan, 'warm', None):
    with pytest.raises(ValueError):
      uisrnn_amd.speaker_posteriors(losses, temperature=bad)
