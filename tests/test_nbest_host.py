"""The n-best readout's CPU side: the replay the GPU tests compare with, and the argument checks.

tests/nbest_ref.py rebuilds every rank's history from the oracle's candidate scores.  Checked here
against what the oracle itself hands out (rank 0's labels, the final beam's scores) and against a
case with a known answer: a beam of Bell(N) hypotheses never prunes, so the final beam is exactly
the set of restricted-growth strings of length N.  No GPU needed.
"""

import numpy as np
import pytest

import golden_util
import nbest_ref
import uisrnn_amd
from uisrnn_amd import uisrnn as host

CONFIGS = [(10, 1, 1), (10, 1, 2), (3, 1, 2), (6, 1, 2), (6, 2, 2), (4, 2, 1), (4, 3, 1), (5, 2, 2)]


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def restricted_growth_strings(n):
  """Every set partition of n frames as a labeling in first-appearance form."""
  out = [[0]] if n else [[]]
  for _ in range(1, n):
    out = [s + [c] for s in out for c in range(max(s) + 2)]
  return sorted(tuple(s) for s in out)


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2', 'd32_lookahead3'])
def test_replay_reproduces_the_oracle(name, oracle_lib):
  case = golden_util.load_case(name)
  seqs = case['seqs'][:2]
  for beam, look, tau in CONFIGS:
    ref = oracle_lib.decode(case['params'], seqs, beam, look, tau, n_threads=2)
    for u, seq in enumerate(seqs):
      rows, scores = nbest_ref.nbest(nbest_ref.replay(case['params'], seq, beam, look, tau))
      assert np.array_equal(rows[0], ref['labels'][u]), (beam, look, tau, u)
      want = ref['beam_scores'][u]
      assert np.array_equal(_bits(scores), _bits(want[:scores.size])), (beam, look, tau, u)
      assert np.all(np.isinf(want[scores.size:]))
      assert np.all(np.diff(scores) >= 0)


@pytest.mark.parametrize('name,n,beam', [('tiny_d16', 4, 15), ('tiny_d16', 5, 52), ('tracker_d256', 4, 15)])
def test_a_beam_of_bell_n_keeps_every_partition(name, n, beam, oracle_lib):
  case = golden_util.load_case(name)
  seq = case['seqs'][0][:n]
  rows, scores = nbest_ref.nbest(nbest_ref.replay(case['params'], seq, beam, 1, 1))
  assert sorted(tuple(r) for r in rows.tolist()) == restricted_growth_strings(n)
  assert rows.shape[0] == beam and np.all(np.diff(scores) >= 0)


def test_prefix_replay_equals_a_replay_of_the_prefix(oracle_lib):
  case = golden_util.load_case('tiny_d16')
  seq = case['seqs'][0][:12]
  whole = nbest_ref.replay(case['params'], seq, 3, 1, 1)
  for n in (1, 5, 12):
    rows, scores = nbest_ref.nbest(whole, upto=n)
    rows2, scores2 = nbest_ref.nbest(nbest_ref.replay(case['params'], seq[:n], 3, 1, 1))
    assert np.array_equal(rows, rows2) and np.array_equal(_bits(scores), _bits(scores2))
  assert nbest_ref.common_prefix(np.array([[0, 1, 1], [0, 1, 2]])) == 2
  assert nbest_ref.common_prefix(np.array([[0, 1, 1]])) == 3
  assert nbest_ref.common_prefix(np.zeros((0, 4), dtype=np.int32)) == 0


def test_predict_nbest_argument_errors_need_no_device():
  model_args, _, inference_args = uisrnn_amd.parse_arguments([])
  model_args.observation_dim = 16
  model = uisrnn_amd.UISRNN(model_args)  # (never fit or loaded: reaching the decoder would raise TypeError)
  seq = np.zeros((5, 16))
  inference_args.beam_size = 4
  for bad in (0, -1, 5, 2.0, True, '2'):
    with pytest.raises(ValueError):
      model.predict_nbest(seq, inference_args, n_best=bad)
    with pytest.raises(ValueError):
      model.predict_nbest([seq], inference_args, n_best=bad)
  # predict's own checks, in predict's words
  with pytest.raises(TypeError, match='either a list or numpy array'):
    model.predict_nbest('nope', inference_args)
  with pytest.raises(TypeError, match='numpy array of float type'):
    model.predict_nbest(seq.astype(np.float32), inference_args, n_best=2)
  with pytest.raises(ValueError, match='2-dim'):
    model.predict_nbest([np.zeros(5)], inference_args, n_best=2)
  assert model.predict_nbest([], inference_args) == []


def test_online_session_nbest_argument_errors_need_no_device():
  session = host.OnlineSession.__new__(host.OnlineSession)  # (no handle: the checks come first)
  session._beam_size = 4
  session._decoder = None
  for bad in (0, 5, -3, 1.5, True):
    with pytest.raises(ValueError):
      session.nbest(bad)
