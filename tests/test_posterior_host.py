"""The posterior readout's CPU side: the reference the GPU tests compare with (tests/posterior_ref.py), the two
symbols, and the argument checks that come before any device work.  No GPU needed.
"""

import ctypes
import os
import subprocess

import numpy as np
import pytest

import golden_util
import nbest_ref
import posterior_ref
import uisrnn_amd
from uisrnn_amd import _capi
from uisrnn_amd import build as lib_build
from uisrnn_amd import uisrnn as host

_BAD_TEMPERATURES = (0, 0.0, -1, -0.5, float('nan'), float('inf'), -float('inf'), '1', None, True, [1.0])


def test_the_references_own_properties(oracle_lib):
  case = golden_util.load_case('tiny_d16')
  seq = case['seqs'][0]
  for beam, tau in ((10, 1), (3, 2)):
    rows, scores = nbest_ref.nbest(nbest_ref.replay(case['params'], seq, beam, 1, tau))
    live = rows.shape[0]
    assert live > 1
    for temperature in (1.0, 4.0):
      conf, change, w = posterior_ref.posterior(rows, scores, temperature)
      assert conf.shape == change.shape == (len(seq),) and w.shape == (live,)
      assert abs(w.sum() - 1.0) < 1e-12 and np.all(np.diff(w) <= 0) and w[0] == w.max()
      assert np.all(conf >= w[0] - 1e-12) and np.all(conf <= 1.0 + 1e-12)
      assert np.all(change >= 0.0) and np.all(change <= 1.0 + 1e-12)
      prefix = nbest_ref.common_prefix(rows)
      assert prefix >= 1 and np.all(np.abs(conf[:prefix] - 1.0) < 1e-12)
      assert change[0] == 0.0
    # a hotter temperature flattens the weights
    assert posterior_ref.posterior(rows, scores, 4.0)[2][0] < posterior_ref.posterior(rows, scores, 1.0)[2][0]
    # the condition the GPU parity tests put on their cases holds here
    conf, change, _ = posterior_ref.posterior(rows, scores, 1.0)
    assert posterior_ref.interior(conf) and posterior_ref.interior(change)
    # one live hypothesis: exact
    conf, change, w = posterior_ref.posterior(rows[:1], scores[:1], 1.0)
    assert w.tolist() == [1.0] and np.all(conf == 1.0)
    want = np.concatenate([[0.0], (rows[0, 1:] != rows[0, :-1]).astype(np.float64)])
    assert np.array_equal(change, want)
  # none
  conf, change, w = posterior_ref.posterior(np.zeros((0, 5), dtype=np.int32), np.zeros(0, dtype=np.float32), 1.0)
  assert conf.tolist() == [0.0] * 5 and change.tolist() == [0.0] * 5 and w.size == 0


def test_a_hand_made_beam():
  rows = np.array([[0, 0, 1, 1], [0, 1, 1, 1], [0, 0, 0, 0]], dtype=np.int32)
  scores = np.array([1.0, 1.0 + np.log(2.0), 1.0 + np.log(4.0)], dtype=np.float32)
  conf, change, w = posterior_ref.posterior(rows, scores, 1.0)
  assert np.allclose(w, [4 / 7, 2 / 7, 1 / 7], atol=1e-7)
  assert np.allclose(conf, [1.0, 5 / 7, 6 / 7, 6 / 7], atol=1e-7)
  assert np.allclose(change, [0.0, 2 / 7, 4 / 7, 0.0], atol=1e-7)
  assert posterior_ref.tolerance(3) == 11 * 2.0 ** -23


def test_the_symbols_are_declared_bound_and_exported():
  root = os.path.join(os.path.dirname(golden_util.GOLDEN_DIR), '..')
  header = open(os.path.join(root, 'include', 'uisrnn_hip.h')).read()
  assert ('int32_t uis_last_decode_posterior(uis_handle* h, double temperature, float* confidence_out, float* change_out,\n'
          '                                  int64_t capacity, float* weights_out, int32_t* counts_out);') in header
  assert ('int32_t uis_stream_posterior(uis_handle* h, double temperature, float* confidence_out, float* change_out,\n'
          '                             int64_t capacity, float* weights_out, int32_t* counts_out);') in header
  lib = lib_build.OUTPUT
  if not os.path.exists(lib):
    lib = lib_build.build()
  symbols = subprocess.run(['nm', '-D', '--defined-only', lib], check=True, capture_output=True, text=True).stdout
  defined = {line.split()[-1] for line in symbols.splitlines() if line.strip()}
  for name in ('uis_last_decode_posterior', 'uis_stream_posterior'):
    assert name in _capi.EXPORTED_SYMBOLS and name in defined
    fn = getattr(_capi.load_library(), name)
    assert fn.argtypes[1] is ctypes.c_double and len(fn.argtypes) == 7
  assert hasattr(_capi.Decoder, 'last_posterior') and hasattr(_capi.Decoder, 'stream_posterior')
  assert hasattr(uisrnn_amd.UISRNN, 'predict_posteriors')
  assert hasattr(host.OnlineSession, 'posteriors') and hasattr(host.StreamPool, 'posteriors')


def test_without_a_handle_the_calls_refuse_and_write_nothing():
  lib = _capi.load_library()
  for fn in (lib.uis_last_decode_posterior, lib.uis_stream_posterior):
    conf = np.full(4, -7.0, dtype=np.float32)
    counts = np.full(2, -7, dtype=np.int32)
    rc = fn(None, 1.0, conf.ctypes.data_as(_capi._fp), None, 4, None, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    assert rc == _capi.UIS_ERR_INVALID_ARG and 'null handle' in _capi.last_error(lib)
    assert (conf == -7.0).all() and (counts == -7).all()


def test_predict_posteriors_argument_errors_need_no_device():
  model_args, _, inference_args = uisrnn_amd.parse_arguments([])
  model_args.observation_dim = 16
  model = uisrnn_amd.UISRNN(model_args)  # (never fit or loaded: reaching the decoder would raise TypeError)
  seq = np.zeros((5, 16))
  for bad in _BAD_TEMPERATURES:
    with pytest.raises(ValueError, match='temperature'):
      model.predict_posteriors(seq, inference_args, temperature=bad)
    with pytest.raises(ValueError, match='temperature'):
      model.predict_posteriors([seq], inference_args, temperature=bad)
  # predict's own checks, in predict's words
  with pytest.raises(TypeError, match='either a list or numpy array'):
    model.predict_posteriors('nope', inference_args)
  with pytest.raises(TypeError, match='numpy array of float type'):
    model.predict_posteriors(seq.astype(np.float32), inference_args, temperature=2)
  assert model.predict_posteriors([], inference_args, temperature=np.float32(2.5)) == []


def test_session_posteriors_argument_errors_need_no_device():
  session = host.OnlineSession.__new__(host.OnlineSession)  # (no handle: the checks come first)
  session._beam_size = 4
  session._decoder = None
  session._num_utterances = 1
  pool = host.StreamPool(session)
  pool.open('a')
  for bad in _BAD_TEMPERATURES:
    with pytest.raises(ValueError, match='temperature'):
      session.posteriors(bad)
    with pytest.raises(ValueError, match='temperature'):
      pool.posteriors('a', temperature=bad)


class _StandIn:
  """A decoder that answers stream_posterior from a table (no library, no device)."""

  def __init__(self, status=0):
    self.status = status
    self.asked = []

  def stream_posterior(self, temperature):
    self.asked.append(temperature)
    return {'confidence': [np.array([1.0, 0.75], dtype=np.float32), np.zeros(0, dtype=np.float32)],
            'change': [np.array([0.0, 0.25], dtype=np.float32), np.zeros(0, dtype=np.float32)],
            'weights': np.array([[0.75, 0.25, 0.0], [1.0, 0.0, 0.0]], dtype=np.float32),
            'counts': np.array([2, 1], dtype=np.int32), 'status': self.status}

  def stream_labels(self):
    return [np.zeros(2, dtype=np.int32), np.zeros(0, dtype=np.int32)], None, np.array([1, 0], dtype=np.int32), self.status


def test_session_posteriors_shape_and_the_cap_error():
  session = host.OnlineSession.__new__(host.OnlineSession)
  session._decoder = _StandIn()
  session._num_utterances = 2
  session._final = [[], [0, 0]]
  got = session.posteriors(np.float64(4))
  assert session._decoder.asked == [4.0] and isinstance(session._decoder.asked[0], float)
  assert [g[0].tolist() for g in got] == [[1.0, 0.75], []] and [g[1].tolist() for g in got] == [[0.0, 0.25], []]
  assert [g[2].tolist() for g in got] == [[0.75, 0.25], [1.0]]      # the live weights only
  pool = host.StreamPool(session)
  pool.open('a')
  pool.open('b')
  assert pool.posteriors('b', 2)[2].tolist() == [1.0]
  session._decoder = _StandIn(_capi.UIS_ERR_CLUSTER_CAP)
  with pytest.raises(RuntimeError, match='need more than max_clusters'):
    session.posteriors()
