"""tests/train_ref.py against the reference's recorded fit(), without a GPU.

The float64 helper is what tests/test_gpu_train_edges.py holds the device to; here it is held to
tests/golden/training/*.npz (the reference's own float32 run) with the bounds tests/test_gpu_train.py
uses for the device: iteration-0 gradients within 1e-4 norm-relative per tensor and losses within
1e-5; 20 iterations of gradients, clip and Adam within 1e-3 of the final weights, loss1 within 1e-3
at every iteration.
"""

import numpy as np
import pytest

import test_train_host as host
import train_ref
from uisrnn_amd import training

CASES = ('d16_h8', 'd2_h8_l2', 'd20_h24_l3')
GRAD_MAX_NORM = 5.0


def _rel(a, b):
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _iteration(flat, z, sub, idx):
  dim, hidden, depth = int(z['dim']), int(z['hidden']), int(z['depth'])
  params = train_ref.unflatten(flat, dim, hidden, depth)
  padded = training.padded_batch(sub, idx)
  lengths = [len(sub[i]) + 1 for i in idx]
  return train_ref.reference(params, padded, lengths, {})


@pytest.mark.parametrize('name', CASES)
def test_iteration0_matches_the_recording(name):
  z, seqs, ids = host.load_case(name)
  dim, hidden, depth = int(z['dim']), int(z['hidden']), int(z['depth'])
  sub, batches = host.seeded_batches(z, seqs, ids, 1)
  ref = _iteration(z['init_flat'], z, sub, batches[0])
  np.testing.assert_allclose(ref.losses, z['losses'][0], rtol=1e-5)
  clipped = train_ref.clip(ref.flat, train_ref.n_rnn(dim, hidden, depth), GRAD_MAX_NORM)
  assert len(clipped) == len(z['grad_flat'])
  for seg_name, sl, shape in ref.segments:
    assert shape[0] * shape[1] == sl.stop - sl.start
    assert _rel(clipped[sl], z['grad_flat'][sl]) <= 1e-4, (seg_name, _rel(clipped[sl], z['grad_flat'][sl]))


@pytest.mark.parametrize('name', CASES)
def test_twenty_iterations_land_on_the_recording(name):
  z, seqs, ids = host.load_case(name)
  dim, hidden, depth = int(z['dim']), int(z['hidden']), int(z['depth'])
  iterations = int(z['iterations'])
  sub, batches = host.seeded_batches(z, seqs, ids, iterations)
  segs = train_ref.segments(dim, hidden, depth)
  n_rnn = train_ref.n_rnn(dim, hidden, depth)
  flat = np.asarray(z['init_flat'], np.float64)
  grads, loss1 = [], []
  for idx in batches:
    ref = _iteration(flat, z, sub, idx)
    loss1.append(ref.losses[1])
    grads.append(train_ref.clip(ref.flat, n_rnn, GRAD_MAX_NORM))
    # the replay of all gradients so far: the moments are rebuilt from the start each time
    flat = train_ref.adam_replay(z['init_flat'], grads, float(z['learning_rate']), len(flat), segs[-1][1])[-1]
  np.testing.assert_allclose(loss1, z['losses'][:, 1], rtol=1e-3)
  for seg_name, sl, _ in segs:
    assert _rel(flat[sl], z['final_flat'][sl]) <= 1e-3, (seg_name, _rel(flat[sl], z['final_flat'][sl]))


def test_clip_and_adam_by_hand():
  """clip: coefficient max_norm / (norm + 1e-6) over the first n_rnn elements only.  adam_replay: the
  first step moves every element with a non-zero gradient by lr against its sign; the clamp; n_adam."""
  g = np.array([3.0, 4.0, 7.0, -2.0])
  out = train_ref.clip(g, 2, 2.5)
  np.testing.assert_allclose(out, [3.0 * 2.5 / (5.0 + 1e-6), 4.0 * 2.5 / (5.0 + 1e-6), 7.0, -2.0], rtol=1e-15)
  assert np.array_equal(train_ref.clip(g, 2, 10.0), g)
  p0 = np.array([1.0, -1.0, 0.5, 0.25, 9.0])
  steps = train_ref.adam_replay(p0, [np.array([2.0, -3.0, 0.0, 1.0, 1.0])], 0.5, 4, slice(3, 5))
  assert len(steps) == 1
  np.testing.assert_allclose(steps[0], [0.5, -0.5, 0.5, 1e-6, 9.0], rtol=1e-7)
  two = train_ref.adam_replay(p0, [np.array([2.0, -3.0, 0.0, 1.0, 1.0])] * 2, 0.5, 4, slice(3, 5))
  # constant gradients: m / sqrt(v) stays at sign(g) after bias correction
  np.testing.assert_allclose(two[1][:2], [0.0, 0.0], atol=1e-7)
