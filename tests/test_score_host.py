"""score_labels without a GPU: the argument checks and the CPU restatement of the contract."""

import ctypes

import numpy as np
import pytest

import forced_ref
import golden_util
import uisrnn_amd
from uisrnn_amd import _capi


def _model(**over):
  model_args, _, _ = uisrnn_amd.parse_arguments([])
  model_args.observation_dim = 16
  model_args.rnn_hidden_size = 8
  model_args.transition_bias = 0.2
  model_args.sigma2 = 0.05
  for key, val in over.items():
    setattr(model_args, key, val)
  return uisrnn_amd.UISRNN(model_args)


def test_score_labels_argument_errors_before_any_device(monkeypatch):
  """The reference's messages (_check_sequence), ValueError for mismatched lengths, TypeError for an
  untrained model -- all raised before a decoder handle is created."""
  def no_device(*args, **kwargs):
    raise AssertionError('a device handle was requested')
  monkeypatch.setattr(_capi, 'Decoder', no_device)
  model = _model()
  seq = np.zeros((4, 16))
  with pytest.raises(TypeError, match='test_sequence should be a numpy array of float type.'):
    model.score_labels(np.zeros((4, 16), dtype=np.float32), [0] * 4)
  with pytest.raises(ValueError, match='test_sequence must be 2-dim array.'):
    model.score_labels(np.zeros(16), [0])
  with pytest.raises(ValueError, match='does not match the dimension specified by args.observation_dim'):
    model.score_labels(np.zeros((4, 15)), [0] * 4)
  with pytest.raises(TypeError, match='test_sequences should be either a list or numpy array.'):
    model.score_labels('abc', [0])
  with pytest.raises(ValueError):
    model.score_labels(seq, [0] * 3)
  with pytest.raises(ValueError):
    model.score_labels([seq, seq], [[0] * 4])
  with pytest.raises(ValueError):
    model.score_labels([seq, np.zeros((2, 3))], [[0] * 4, [0] * 2])
  with pytest.raises(TypeError, match='test_sequence should be a numpy array of float type.'):
    model.score_labels([[[1.0] * 16]], [[0]])
  with pytest.raises(TypeError, match='transition_bias is None'):
    _model(transition_bias=None).score_labels(seq, [0] * 4)


def test_score_labels_c_abi_rejects_bad_arguments_without_a_device():
  lib = _capi.load_library()
  off = np.array([0, 2], dtype=np.int64)
  lab = np.array([0, -1], dtype=np.int32)
  rc = lib.uis_score_labels(None, None, off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1,
                            lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None, None)
  assert rc == _capi.UIS_ERR_INVALID_ARG


def test_first_appearance_renaming():
  assert forced_ref.first_appearance(['b', 'a', 'b', 'c']).tolist() == [0, 1, 0, 2]
  assert forced_ref.first_appearance([7, 7, 3]).tolist() == [0, 0, 1]


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2', 'd20_h24_depth3'])
def test_restatement_scores_decoded_labels_like_the_oracle_decode(name, oracle_lib):
  """The main correctness statement on the CPU side: the labels a test_iteration 1 decode returns
  score, along the fixed trace, exactly the decode's best score."""
  case = golden_util.load_case(name)
  params, seqs = case['params'], case['seqs']
  for beam, look_ahead in ((1, 1), (4, 1), (3, 2)):
    ref = oracle_lib.decode(params, seqs, beam, look_ahead, 1)
    got, losses = forced_ref.score(params, seqs, ref['labels'])
    assert np.array_equal(got.view(np.uint32), ref['scores'].view(np.uint32)), (beam, look_ahead, got, ref['scores'])
    for u, per in enumerate(losses):
      acc = np.float32(0.0)
      for v in per:
        acc = np.float32(acc + v)
      assert acc.view(np.uint32) == got[u].view(np.uint32)


def test_restatement_invalid_trace_is_inf(oracle_lib):
  case = golden_util.load_case('tiny_d16')
  seq = case['seqs'][0][:6]
  score, losses = forced_ref.score_one(case['params'], seq, [0, 1, 3, 0, 0, 0])
  assert np.isposinf(score) and np.all(np.isposinf(losses[2:])) and np.all(np.isfinite(losses[:2]))
