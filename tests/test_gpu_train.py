"""train() on the MI355X against the reference's own fit() (tests/golden/make_training.py).

  * gradient parity: iteration 0's gradients (post-clip, rnn_init_hidden and sigma2 included)
    within 1e-4 of the reference's, norm-relative per tensor; that iteration's losses within 1e-5
  * trajectory: 20 iterations from the reference's starting weights and seeds, loss1 within 1e-3
    relative at every iteration, final weights within 1e-3 norm-relative per tensor
  * the reference's own behavioural tests through train(): one training label (uisrnn_test.py),
    four clusters on a square with depth 2 and dropout (integration_test.py)
  * determinism, save / load, predict after train()
"""

import random

import numpy as np
import pytest

import test_train_host as host
from train_ref import dropout_scales
from train_ref import torch_gradients as _torch_gradients
from tools import train_behaviour
import uisrnn_amd
from uisrnn_amd import _capi
from uisrnn_amd import weights

pytestmark = pytest.mark.gpu

CASES = host.CASES


def _like(dim, hidden, depth):
  return weights.init_params(dim, hidden, depth, transition_bias=0.5)


def _segments(like):
  """(name, flat slice) of every tensor in the trainer's flat order."""
  out, pos = [], 0
  names = []
  for l in range(int(like['rnn_depth'])):
    for key in ('gru_weight_ih', 'gru_weight_hh', 'gru_bias_ih', 'gru_bias_hh'):
      names.append(('{}[{}]'.format(key, l), np.size(like[key][l])))
  for key in ('linear_mean1_weight', 'linear_mean1_bias', 'linear_mean2_weight',
              'linear_mean2_bias', 'rnn_init_hidden', 'sigma2'):
    names.append((key, np.size(like[key])))
  for name, n in names:
    out.append((name, slice(pos, pos + n)))
    pos += n
  return out


def _initial_flat(z):
  """The reference's starting weights: recorded, or rebuilt with torch from the seed (D 256)."""
  dim, hidden, depth = int(z['dim']), int(z['hidden']), int(z['depth'])
  if 'init_flat' in z:
    return z['init_flat']
  import torch  # pylint: disable=import-outside-toplevel
  torch.manual_seed(int(z['seeds'][2]))
  mods = [torch.nn.GRU(dim, hidden, depth), torch.nn.Linear(hidden, hidden), torch.nn.Linear(hidden, dim)]
  parts = [p.detach().numpy().ravel() for m in mods for p in m.parameters()]
  parts += [np.zeros(depth * hidden, np.float32), np.full(dim, 0.1, np.float32)]
  flat = np.concatenate(parts).astype(np.float32)
  assert np.array_equal(flat[z['sample_idx']], z['init_val'])
  return flat


def _args(z, iterations):
  model_args, training_args, inference_args = uisrnn_amd.parse_arguments([])
  model_args.observation_dim = int(z['dim'])
  model_args.rnn_hidden_size = int(z['hidden'])
  model_args.rnn_depth = int(z['depth'])
  model_args.rnn_dropout = 0.0
  model_args.verbosity = 0
  training_args.learning_rate = float(z['learning_rate'])
  training_args.batch_size = int(z['batch_size'])
  training_args.train_iteration = iterations
  return model_args, training_args, inference_args


def _rel(a, b):
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.mark.parametrize('name', CASES)
def test_iteration0_gradients_match_the_reference(name):
  z, seqs, ids = host.load_case(name)
  dim, hidden, depth = int(z['dim']), int(z['hidden']), int(z['depth'])
  like = _like(dim, hidden, depth)
  init = _initial_flat(z)
  sub, batches = host.seeded_batches(z, seqs, ids, 1)
  trainer = _capi.Trainer(_capi.unflatten_params(init, like), learning_rate=float(z['learning_rate']),
                          estimate_sigma2=True)
  try:
    trainer.set_data(sub)
    losses = trainer.step(batches[0])
    grads = trainer.flat_grads()
  finally:
    trainer.close()
  np.testing.assert_allclose(losses, z['losses'][0], rtol=1e-5)
  if 'grad_flat' in z:
    for seg_name, sl in _segments(like):
      assert _rel(grads[sl], z['grad_flat'][sl]) <= 1e-4, (seg_name, _rel(grads[sl], z['grad_flat'][sl]))
  else:
    idx = z['sample_idx']
    assert _rel(grads[idx], z['grad_val']) <= 1e-4, _rel(grads[idx], z['grad_val'])
    assert np.linalg.norm(grads.astype(np.float64)) == pytest.approx(float(z['grad_norm']), rel=1e-4)


@pytest.mark.parametrize('name', CASES)
def test_twenty_iterations_follow_the_reference(name):
  z, seqs, ids = host.load_case(name)
  dim, hidden, depth = int(z['dim']), int(z['hidden']), int(z['depth'])
  model_args, training_args, _ = _args(z, int(z['iterations']))
  model = uisrnn_amd.UISRNN(model_args)
  start = _capi.unflatten_params(_initial_flat(z), _like(dim, hidden, depth))
  start['transition_bias'] = None
  model.load_params(start)
  np.random.seed(int(z['seeds'][0]))
  random.seed(int(z['seeds'][1]))
  model.train([s.copy() for s in seqs], [list(i) for i in ids], training_args)
  loss1 = np.array([r['loss1'] for r in model.last_train_losses])
  np.testing.assert_allclose(loss1, z['losses'][:, 1], rtol=1e-3)
  assert model.transition_bias == pytest.approx(float(z['transition_bias']))
  final = _capi.flatten_params(model.params)
  if 'final_flat' in z:
    for seg_name, sl in _segments(model.params):
      assert _rel(final[sl], z['final_flat'][sl]) <= 1e-3, (seg_name, _rel(final[sl], z['final_flat'][sl]))
  else:
    assert _rel(final[z['sample_idx']], z['final_val']) <= 1e-3


def test_single_label_predicts_zeros():
  """The reference's tests/uisrnn_test.py:26-70, trained here from seeded starting weights."""
  _, one, many, par = train_behaviour.single_label(weight_seed=0)
  assert one == [0] * 10
  assert many == [[0] * 10] * 3
  assert par == [[0] * 10] * 3


def test_four_clusters_depth2_with_dropout(tmp_path):
  """The reference's tests/integration_test.py toy case: depth 2, default dropout, accuracy 1.0.

  Seeded starting weights make it deterministic; tools/train_behaviour.py sweeps the seeds."""
  model, train_data, test_seq, test_id, inference_args, labels = train_behaviour.four_clusters(weight_seed=0)
  assert model.rnn_dropout > 0 and model.params['rnn_depth'] == 2
  assert len(model.last_train_losses) == 200
  assert uisrnn_amd.compute_sequence_match_accuracy(labels, test_id) == 1.0
  path = str(tmp_path / 'toy.uisrnn')
  model.save(path)
  model_args, _, _ = uisrnn_amd.parse_arguments([])
  model_args.rnn_depth, model_args.rnn_hidden_size, model_args.observation_dim = 2, 8, 2
  loaded = uisrnn_amd.UISRNN(model_args)
  loaded.load(path)
  labels = loaded.predict(test_seq, inference_args)
  assert uisrnn_amd.compute_sequence_match_accuracy(labels, test_id) == 1.0
  # a further train() merges a new transition_bias estimate
  train_seqs, _, training_args = train_data
  bias = loaded.transition_bias
  training_args.train_iteration = 2
  loaded.train(train_seqs[:1], [['A', 'B'] * 50], training_args)
  assert loaded.transition_bias != bias


@pytest.mark.parametrize('p', [0.0, 0.4])
def test_dropout_gradients_match_autograd(p):
  """depth 2 with dropout: the trainer's gradients against float64 torch autograd fed the trainer's
  own masks (recomputed here from the key), per tensor within 1e-4 norm-relative."""
  z, seqs, ids = host.load_case('d2_h8_l2')
  like = _like(int(z['dim']), int(z['hidden']), int(z['depth']))
  params = _capi.unflatten_params(_initial_flat(z), like)
  sub, batches = host.seeded_batches(z, seqs, ids, 1)
  idx = batches[0]
  key = 0x0123456789abcdef
  trainer = _capi.Trainer(params, learning_rate=float(z['learning_rate']), grad_max_norm=1e30,
                          estimate_sigma2=True, dropout=p, dropout_key=key)
  try:
    trainer.set_data(sub)
    losses = trainer.step(idx)
    grads = trainer.flat_grads()
  finally:
    trainer.close()
  padded = host.training.padded_batch(sub, idx)
  lengths = [len(sub[i]) + 1 for i in idx]
  n = padded.shape[0] * padded.shape[1] * int(z['hidden'])
  masks = {1: dropout_scales(key, 0, 1, n, p)}
  if p > 0:
    dropped = float(np.mean(masks[1] == 0))
    assert 0.3 < dropped < 0.5, dropped
  ref, ref_losses = _torch_gradients(params, padded, lengths, masks)
  np.testing.assert_allclose(losses, ref_losses, rtol=1e-5)
  for seg_name, sl in _segments(like):
    assert _rel(grads[sl], ref[sl]) <= 1e-4, (seg_name, _rel(grads[sl], ref[sl]))


def test_depth1_train_leaves_pythons_random_as_the_reference_does():
  """Without dropout train() draws Python's random exactly as the reference's fit() does."""
  z, seqs, ids = host.load_case('d16_h8')
  model_args, training_args, _ = _args(z, 2)
  model = uisrnn_amd.UISRNN(model_args)
  np.random.seed(5)
  random.seed(5)
  model.train([s.copy() for s in seqs], [list(i) for i in ids], training_args)
  after_train = random.random()
  random.seed(5)
  host.training.concatenate_training_data([s.copy() for s in seqs], [list(i) for i in ids], True, True)
  assert after_train == random.random()


def _small_run(seed):
  z, seqs, ids = host.load_case('d20_h24_l3')
  model_args, training_args, _ = _args(z, 5)
  model_args.rnn_dropout = 0.3
  model = uisrnn_amd.UISRNN(model_args)
  start = _capi.unflatten_params(z['init_flat'], _like(int(z['dim']), int(z['hidden']), int(z['depth'])))
  start['transition_bias'] = None
  model.load_params(start)
  np.random.seed(seed)
  random.seed(seed)
  model.train([s.copy() for s in seqs], [list(i) for i in ids], training_args)
  return model


def test_training_is_deterministic():
  a = _capi.flatten_params(_small_run(7).params)
  b = _capi.flatten_params(_small_run(7).params)
  assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_full_batch_runs():
  z, seqs, ids = host.load_case('d16_h8')
  model_args, training_args, _ = _args(z, 3)
  training_args.batch_size = None
  model = uisrnn_amd.UISRNN(model_args)
  model.train([s.copy() for s in seqs], [list(i) for i in ids], training_args)
  assert all(np.isfinite(r['loss']) for r in model.last_train_losses)


def test_save_and_predict_use_the_trained_weights(tmp_path):
  z, seqs, ids = host.load_case('d16_h8')
  model_args, training_args, inference_args = _args(z, 10)
  model = uisrnn_amd.UISRNN(model_args)
  before = _capi.flatten_params(model.params)
  model.transition_bias = 0.3
  first = model.predict(seqs[0], inference_args)  # builds the decoder on the initial weights
  del first
  model.train([s.copy() for s in seqs], [list(i) for i in ids], training_args)
  after = _capi.flatten_params(model.params)
  assert not np.array_equal(before, after)
  path = str(tmp_path / 'trained.uisrnn')
  model.save(path)
  back = weights.load_checkpoint(path)
  assert np.array_equal(_capi.flatten_params(back), after)
  fresh = uisrnn_amd.UISRNN(model_args)
  fresh.load(path)
  assert model.predict(seqs[0], inference_args) == fresh.predict(seqs[0], inference_args)
  dec = _capi.Decoder(model.params)
  m0, _ = dec.constants()
  assert np.array_equal(model._get_decoder().constants()[0], m0)  # pylint: disable=protected-access
