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


M64 = (1 << 64) - 1


def _mix64(x):
  """uis_train.hip's mix64 on a uint64 array."""
  with np.errstate(over='ignore'):
    x = x + np.uint64(0x9e3779b97f4a7c15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return x ^ (x >> np.uint64(31))


def dropout_scales(key, iteration, layer, n, p):
  """The trainer's dropout multipliers for the n outputs of layer-1 feeding `layer` (include/uisrnn_hip.h)."""
  salt = _mix64(np.array([(iteration * 0x100000001b3 + layer) & M64], dtype=np.uint64))[0]
  h = _mix64(np.uint64(key) ^ salt ^ _mix64(np.arange(n, dtype=np.uint64)))
  u = (h >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
  return np.where(u >= np.float32(p), np.float32(1.0) / (np.float32(1.0) - np.float32(p)), np.float32(0.0))


def _torch_gradients(params, padded, lengths, masks, reg=1e-5, alpha=1.0, beta=1.0):
  """Iteration-0 gradients of the reference's loss in float64 torch (CPU), the given dropout masks
  between layers, no clipping; flat order of the trainer."""
  import torch  # pylint: disable=import-outside-toplevel
  from torch import nn  # pylint: disable=import-outside-toplevel
  t64 = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
  depth, hid, dim = params['rnn_depth'], params['rnn_hidden_size'], params['observation_dim']
  grus = []
  for l in range(depth):
    gru = nn.GRU(dim if l == 0 else hid, hid, 1).double()
    with torch.no_grad():
      gru.weight_ih_l0.copy_(t64(params['gru_weight_ih'][l]))
      gru.weight_hh_l0.copy_(t64(params['gru_weight_hh'][l]))
      gru.bias_ih_l0.copy_(t64(params['gru_bias_ih'][l]))
      gru.bias_hh_l0.copy_(t64(params['gru_bias_hh'][l]))
    grus.append(gru)
  lin1, lin2 = nn.Linear(hid, hid).double(), nn.Linear(hid, dim).double()
  with torch.no_grad():
    lin1.weight.copy_(t64(params['linear_mean1_weight']))
    lin1.bias.copy_(t64(params['linear_mean1_bias']))
    lin2.weight.copy_(t64(params['linear_mean2_weight']))
    lin2.bias.copy_(t64(params['linear_mean2_bias']))
  h0 = nn.Parameter(t64(params['rnn_init_hidden']).view(depth, 1, hid))
  sigma2 = nn.Parameter(t64(params['sigma2']))
  x = t64(padded)
  seq = x
  for l, gru in enumerate(grus):
    if l > 0:
      seq = seq * t64(masks[l]).view(seq.shape)
    packed = nn.utils.rnn.pack_padded_sequence(seq, lengths)
    out, _ = gru(packed, h0[l:l + 1].repeat(1, x.shape[1], 1))
    seq, _ = nn.utils.rnn.pad_packed_sequence(out, total_length=x.shape[0])
  mean = lin2(torch.relu(lin1(seq)))
  mean = torch.cumsum(mean, dim=0) / torch.arange(1, mean.shape[0] + 1).double().view(-1, 1, 1)
  truth = x[1:]
  sq = (((truth != 0).double() * mean[:-1] - truth) ** 2).view(-1, dim)
  n_d = (sq != 0).double().sum(dim=0)
  loss1 = (sq / (2 * sigma2)).sum() / (sq[:, 0] != 0).double().sum()
  loss2 = ((2 * alpha + n_d + 2) / (2 * n_d) * torch.log(sigma2)).sum() + (beta / (sigma2 * n_d)).sum()
  rnn_params = [p for g in grus for p in g.parameters()] + list(lin1.parameters()) + list(lin2.parameters())
  loss3 = reg * sum(torch.norm(p) for p in rnn_params)
  (loss1 + loss2 + loss3).backward()
  grads = [p.grad.numpy().ravel() for p in rnn_params] + [h0.grad.numpy().ravel(), sigma2.grad.numpy().ravel()]
  losses = [loss1 + loss2 + loss3, loss1, loss2, loss3]
  return np.concatenate(grads), [float(v.detach()) for v in losses]


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
