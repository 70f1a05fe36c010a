"""train(): the host half, without a GPU.

Data preparation must draw Python's `random` and the global `np.random` exactly as the
reference's fit() does, so that a seeded caller gets the reference's batches; the fixtures
(tests/golden/make_training.py) record the reference's padded batch of every iteration.
"""

import os
import random

import numpy as np
import pytest

import uisrnn_amd
from uisrnn_amd import synth
from uisrnn_amd import training

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = ('d16_h8', 'd2_h8_l2', 'd20_h24_l3', 'd256_h512')


def load_case(name):
  """(fixture, training sequences, their labels)."""
  z = np.load(os.path.join(GOLDEN, 'training', '{}.npz'.format(name)))
  if 'synth_seed' in z:
    seqs, ids = synth.make_utterances(int(z['synth_seed']), 4, 100, 256)
    ids = [['s{}'.format(int(i)) for i in row] for row in ids]
  else:
    n = int(z['n_seqs'])
    seqs = [z['data_seq_{}'.format(u)] for u in range(n)]
    ids = [z['data_ids_{}'.format(u)].tolist() for u in range(n)]
  return z, seqs, ids


def seeded_batches(z, seqs, ids, iterations, batch_size=10, enforce_uniqueness=True):
  """What train() does before the device is involved, from the fixture's seeds."""
  np.random.seed(int(z['seeds'][0]))
  random.seed(int(z['seeds'][1]))
  sequence, labels = training.concatenate_training_data(
      [s.copy() for s in seqs], [list(i) for i in ids], enforce_uniqueness, True)
  sub, plan = training.prepare(sequence, np.array(labels), 10, batch_size)
  return sub, [plan.next() for _ in range(iterations)]


@pytest.mark.parametrize('name', CASES)
def test_batches_match_the_reference(name):
  z, seqs, ids = load_case(name)
  sub, batches = seeded_batches(z, seqs, ids, int(z['iterations']))
  for it, idx in enumerate(batches):
    padded = training.padded_batch(sub, idx)
    lengths = np.array([len(sub[i]) + 1 for i in idx])
    assert np.array_equal(lengths, z['batch_lengths'][it]), it
    assert padded.shape[0] == lengths[0]
    np.testing.assert_allclose(padded.astype(np.float64).sum(axis=(0, 2)), z['batch_colsum'][it],
                               rtol=1e-5, atol=1e-4)


def test_transition_bias_estimate_and_merge():
  z, _, ids = load_case('d16_h8')
  bias, denominator = training.estimate_transition_bias(ids)
  assert bias == pytest.approx(float(z['transition_bias']), rel=1e-12)
  assert denominator == float(z['transition_bias_denominator'])
  # by hand: 2 changes in 5 pairs, smooth 1 -> 3 / 7
  assert training.estimate_transition_bias([['a', 'a', 'b', 'b', 'a', 'a']]) == (3 / 7, 7)
  assert training.estimate_transition_bias([['a']]) == (0.5, 2)
  # a second fit weights its estimate by the denominators
  merged, den = training.merge_transition_bias(0.25, 8, 0.5, 2)
  assert merged == pytest.approx((0.25 * 8 + 0.5 * 2) / 10) and den == 10
  assert training.merge_transition_bias(None, 0.0, 0.3, 4) == (0.3, 4)


def test_full_batch_draws_nothing():
  state = np.random.get_state()[1].copy()
  plan = training.BatchPlan([3, 5, 5, 2], None)
  idx = plan.next()
  assert np.array_equal(np.random.get_state()[1], state)
  assert [[3, 5, 5, 2][i] for i in idx] == [5, 5, 3, 2]


def test_permuted_segments_keep_runs():
  np.random.seed(0)
  out = training.sample_permuted_segments(np.array([1, 2, 6, 10, 11, 12]), 5)
  for s in out:
    assert sorted(s.tolist()) == [1, 2, 6, 10, 11, 12]
    pos = {v: k for k, v in enumerate(s.tolist())}
    assert pos[2] == pos[1] + 1 and pos[11] == pos[10] + 1 and pos[12] == pos[11] + 1
  assert len(training.sample_permuted_segments(np.array([4]), 3)) == 3


def _model(dim=4):
  model_args, training_args, _ = uisrnn_amd.parse_arguments(['--observation_dim', str(dim)])
  return uisrnn_amd.UISRNN(model_args), training_args


def test_train_argument_errors_match_the_reference():
  """Messages of uisrnn/uisrnn.py:214-237 and :349-362, uisrnn/utils.py concatenate_training_data."""
  model, args = _model()
  with pytest.raises(TypeError, match='train_sequence should be a numpy array of float type.'):
    model.train_concatenated(np.zeros((4, 4), dtype=np.float32), ['a'] * 4, args)
  with pytest.raises(TypeError, match='train_cluster_id type be a numpy array of strings.'):
    model.train_concatenated(np.zeros((4, 4)), np.zeros(4), args)
  with pytest.raises(ValueError, match='train_sequence must be 2-dim array.'):
    model.train_concatenated(np.zeros(4), ['a'] * 4, args)
  with pytest.raises(ValueError, match='train_cluster_id must be 1-dim array.'):
    model.train_concatenated(np.zeros((4, 4)), np.array([['a'] * 4]), args)
  with pytest.raises(ValueError, match='does not match the dimension specified by args.observation_dim'):
    model.train_concatenated(np.zeros((4, 3)), ['a'] * 4, args)
  with pytest.raises(ValueError, match='train_sequence length is not equal to train_cluster_id length.'):
    model.train_concatenated(np.zeros((4, 4)), ['a'] * 3, args)
  with pytest.raises(TypeError, match='train_sequences must be a list or numpy.ndarray'):
    model.train('abc', ['a'], args)
  with pytest.raises(ValueError, match='train_sequences and train_cluster_ids must have same size'):
    model.train([np.zeros((4, 4))], [], args)
  with pytest.raises(ValueError, match='train_sequences must have consistent observation dimension'):
    model.train([np.zeros((4, 4)), np.zeros((4, 3))], [['a'] * 4, ['a'] * 4], args)
  with pytest.raises(ValueError, match='Each train_sequence and its train_cluster_id must have same length'):
    model.train([np.zeros((4, 4))], [['a'] * 3], args)
  with pytest.raises(TypeError, match='Elements of train_cluster_ids must be list or numpy.ndarray'):
    model.train([np.zeros((4, 4))], ['abcd'], args)


def test_fit_still_raises():
  model, args = _model()
  with pytest.raises(NotImplementedError):
    model.fit(np.zeros((4, 4)), ['a'] * 4, args)
  with pytest.raises(NotImplementedError):
    model.fit_concatenated(np.zeros((4, 4)), ['a'] * 4, args)
