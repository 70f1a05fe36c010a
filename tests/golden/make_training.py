"""Fixtures for the trainer: the REFERENCE's own fit(), iteration by iteration.

Runs only in the dev container (imports the reference with make_golden.py's shims); the .npz
files it writes under tests/golden/ are what the tests read.

  python tests/golden/make_training.py            # every case
  python tests/golden/make_training.py d16_h8     # one case

Each case seeds np.random / random / torch, builds the reference's UISRNN (torch initialises the
weights) and records into training/<case>.npz (a directory of its own: the decode fixtures' tests list *.npz here):
  seeds            np / random / torch seeds
  init_flat        the starting weights, in the trainer's flat order (include/uisrnn_hip.h);
                   D 256 / H 512: init_idx / init_val, a seeded sample (the test rebuilds the
                   weights with torch from the seed and checks them against the sample)
  data_*           the training sequences and labels (small cases) or their synth seed
  batch_lengths    [iterations, batch] the padded lengths of every iteration's batch
  batch_colsum     [iterations, batch] the sum of each column of that batch's padded input
  losses           [iterations, 4] loss, loss1, loss2, loss3 of a 20-iteration fit
  grad_flat        after a train_iteration=1 fit, every parameter's .grad read off the modules
                   (post-clip; rnn_init_hidden and sigma2 included), flat order
  final_flat       the weights after the 20-iteration fit
D 256 / H 512 records grad and final weights as seeded samples (*_idx / *_val).
"""

import os
import random
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import make_golden  # noqa: E402  pylint: disable=wrong-import-position

ITERATIONS = 20
SAMPLE = 4096

# name: (D, H, depth, batch_size, data)
CASES = {
    'd16_h8': dict(dim=16, hidden=8, depth=1, batch=10, lr=0.01),
    'd2_h8_l2': dict(dim=2, hidden=8, depth=2, batch=10, lr=0.01),
    'd20_h24_l3': dict(dim=20, hidden=24, depth=3, batch=10, lr=0.005),
    'd256_h512': dict(dim=256, hidden=512, depth=1, batch=10, lr=1e-3),
}
SYNTH_SEED = 9000


def make_data(case, cfg):
  """Small cases: a few utterances of random frames with run-length speaker labels."""
  if cfg['dim'] == 256:
    from uisrnn_amd import synth  # pylint: disable=import-outside-toplevel
    seqs, ids = synth.make_utterances(SYNTH_SEED, 4, 100, 256)
    return seqs, [['s{}'.format(int(i)) for i in row] for row in ids]
  rng = np.random.RandomState(zlib.crc32(case.encode()))
  seqs, ids = [], []
  for _ in range(3):
    n = int(rng.randint(30, 60))
    labels, spk = [], 0
    while len(labels) < n:
      labels += ['spk{}'.format(spk)] * int(rng.randint(3, 12))
      spk = int(rng.randint(0, 3))
    labels = labels[:n]
    seqs.append(rng.rand(n, cfg['dim']) + np.array([int(l[3:]) for l in labels])[:, None])
    ids.append(labels)
  return seqs, ids


def seed_all(seeds):
  import torch  # pylint: disable=import-outside-toplevel
  np.random.seed(seeds[0])
  random.seed(seeds[1])
  torch.manual_seed(seeds[2])


def flat_of(model):
  """The reference model's weights in the trainer's flat order."""
  parts = [p.detach().numpy().ravel() for p in model.rnn_model.parameters()]
  parts.append(model.rnn_init_hidden.detach().numpy().ravel())
  parts.append(model.sigma2.detach().numpy().ravel())
  return np.concatenate(parts).astype(np.float32)


def grads_of(model):
  parts = [p.grad.numpy().ravel() for p in model.rnn_model.parameters()]
  parts.append(model.rnn_init_hidden.grad.numpy().ravel())
  parts.append(model.sigma2.grad.numpy().ravel())
  return np.concatenate(parts).astype(np.float32)


def run_case(case):
  import torch  # pylint: disable=import-outside-toplevel
  cfg = CASES[case]
  uisrnn = make_golden.import_reference()
  utils = sys.modules['uisrnn.utils']
  loss_func = sys.modules['uisrnn.loss_func']
  seqs, ids = make_data(case, cfg)
  seeds = (3, 4, 5)

  def model_and_args():
    model_args, training_args, _ = make_golden_args(uisrnn)
    model_args.enable_cuda = False
    model_args.observation_dim = cfg['dim']
    model_args.rnn_hidden_size = cfg['hidden']
    model_args.rnn_depth = cfg['depth']
    model_args.rnn_dropout = 0.0
    model_args.verbosity = 0
    training_args.learning_rate = cfg['lr']
    training_args.batch_size = cfg['batch']
    return model_args, training_args

  record = {'batch_lengths': [], 'batch_colsum': [], 'losses': []}
  orig_pack = utils.pack_sequence
  orig = (loss_func.weighted_mse_loss, loss_func.sigma2_prior_loss, loss_func.regularization_loss)
  cur = {}

  def pack(*a, **kw):
    packed, truth = orig_pack(*a, **kw)
    padded, lengths = torch.nn.utils.rnn.pad_packed_sequence(packed)
    record['batch_lengths'].append(lengths.numpy().astype(np.int32))
    record['batch_colsum'].append(padded.double().sum(dim=(0, 2)).numpy())
    return packed, truth

  def l1(*a, **kw):
    cur['l1'] = orig[0](*a, **kw)
    return cur['l1']

  def l2(*a, **kw):
    cur['l2'] = orig[1](*a, **kw)
    return cur['l2']

  def l3(*a, **kw):
    v = orig[2](*a, **kw)
    total = cur['l1'] + cur['l2'] + v
    record['losses'].append([float(total), float(cur['l1']), float(cur['l2']), float(v)])
    return v

  utils.pack_sequence = pack
  loss_func.weighted_mse_loss, loss_func.sigma2_prior_loss, loss_func.regularization_loss = l1, l2, l3
  try:
    # one iteration: the gradients
    seed_all(seeds)
    model_args, training_args = model_and_args()
    model = uisrnn.UISRNN(model_args)
    init = flat_of(model)
    training_args.train_iteration = 1
    model.fit([s.copy() for s in seqs], [list(i) for i in ids], training_args)
    grads = grads_of(model)
    losses_it1 = list(record['losses'])
    # the trajectory, from the same seeds
    record = {'batch_lengths': [], 'batch_colsum': [], 'losses': []}
    seed_all(seeds)
    model_args, training_args = model_and_args()
    model = uisrnn.UISRNN(model_args)
    assert np.array_equal(flat_of(model), init)
    training_args.train_iteration = ITERATIONS
    model.fit([s.copy() for s in seqs], [list(i) for i in ids], training_args)
    final = flat_of(model)
  finally:
    utils.pack_sequence = orig_pack
    loss_func.weighted_mse_loss, loss_func.sigma2_prior_loss, loss_func.regularization_loss = orig
  assert np.allclose(losses_it1[0], record['losses'][0])
  out = {
      'seeds': np.array(seeds, dtype=np.int64),
      'dim': np.int64(cfg['dim']), 'hidden': np.int64(cfg['hidden']), 'depth': np.int64(cfg['depth']),
      'batch_size': np.int64(cfg['batch']), 'learning_rate': np.float64(cfg['lr']),
      'iterations': np.int64(ITERATIONS),
      'batch_lengths': np.stack(record['batch_lengths']),
      'batch_colsum': np.stack(record['batch_colsum']),
      'losses': np.array(record['losses'], dtype=np.float64),
      'transition_bias': np.float64(model.transition_bias),
      'transition_bias_denominator': np.float64(model.transition_bias_denominator),
  }
  if cfg['dim'] == 256:
    rng = np.random.RandomState(11)
    idx = np.sort(rng.choice(len(init), SAMPLE, replace=False))
    # every rnn_init_hidden and sigma2 entry, and the sample
    tail = len(init) - cfg['depth'] * cfg['hidden'] - cfg['dim']
    idx = np.union1d(idx, np.arange(tail, len(init)))
    out.update({'synth_seed': np.int64(SYNTH_SEED), 'sample_idx': idx.astype(np.int64),
                'init_val': init[idx], 'grad_val': grads[idx], 'final_val': final[idx],
                'grad_norm': np.float64(np.linalg.norm(grads.astype(np.float64)))})
  else:
    out.update({'init_flat': init, 'grad_flat': grads, 'final_flat': final,
                'n_seqs': np.int64(len(seqs))})
    for u, (s, i) in enumerate(zip(seqs, ids)):
      out['data_seq_{}'.format(u)] = s
      out['data_ids_{}'.format(u)] = np.array(i)
  path = os.path.join(HERE, 'training', '{}.npz'.format(case))
  np.savez_compressed(path, **out)
  print(case, os.path.getsize(path), 'bytes; loss1', out['losses'][:3, 1], '...', out['losses'][-1, 1])


def make_golden_args(uisrnn):
  argv = sys.argv
  sys.argv = argv[:1]
  try:
    model_args, training_args, inference_args = uisrnn.parse_arguments()
  finally:
    sys.argv = argv
  return model_args, training_args, inference_args


def main():
  names = sys.argv[1:] or list(CASES)
  for name in names:
    run_case(name)


if __name__ == '__main__':
  main()
