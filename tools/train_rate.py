"""Training rate on the MI355X: the HIP trainer against an equivalent torch-ROCm model.

  python tools/train_rate.py [--iters 200] [--warmup 20] [--utts 40] [--frames 300] [--out FILE]

The 8(d) recipe: synthetic utterances (uisrnn_amd.synth, seeds 5000..), D 256, H 512, depth 1,
batch 10, lr 1e-3, the reference's default num_permutations 10.  Both legs train on the same
batch sequence (one np.random draw per iteration, as the reference).  Times are wall time
around device-synchronised loops after a warm-up.  The torch leg is nn.GRU + two nn.Linear,
the reference's losses, autograd, clip_grad_norm_ and optim.Adam, on cuda:0.

For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python ...` with
--no-torch.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from uisrnn_amd import _capi  # noqa: E402  pylint: disable=wrong-import-position
from uisrnn_amd import synth  # noqa: E402  pylint: disable=wrong-import-position
from uisrnn_amd import training  # noqa: E402  pylint: disable=wrong-import-position
from uisrnn_amd import weights  # noqa: E402  pylint: disable=wrong-import-position


def data(n_utts, frames, dim):
  seqs, ids = synth.make_utterances(5000, n_utts, frames, dim)
  ids = [['s{}'.format(int(i)) for i in row] for row in ids]
  np.random.seed(1)
  import random  # pylint: disable=import-outside-toplevel
  random.seed(1)
  seq, labels = training.concatenate_training_data(seqs, ids, True, True)
  return training.prepare(seq, np.array(labels), 10, 10)


def hip_leg(params, sub, batches, warmup):
  tr = _capi.Trainer(params, learning_rate=1e-3)
  tr.set_data(sub)
  for b in batches[:warmup]:
    tr.step(b)
  t0 = time.perf_counter()
  losses = None
  for b in batches[warmup:]:
    losses = tr.step(b)   # reads the losses back: synchronises every iteration
  dt = time.perf_counter() - t0
  t1 = time.perf_counter()
  for b in batches[warmup:]:
    tr.step(b, want_losses=False)
  tr.flat_params()       # synchronises
  dt_async = time.perf_counter() - t1
  tr.close()
  n = len(batches) - warmup
  return {'ms_per_iter': 1e3 * dt / n, 'ms_per_iter_no_loss_readback': 1e3 * dt_async / n,
          'last_losses': losses}


def torch_leg(params, sub, batches, warmup):
  import torch  # pylint: disable=import-outside-toplevel
  from torch import nn  # pylint: disable=import-outside-toplevel
  dev = torch.device('cuda:0')
  dim, hid = params['observation_dim'], params['rnn_hidden_size']
  gru = nn.GRU(dim, hid, 1).to(dev)
  lin1, lin2 = nn.Linear(hid, hid).to(dev), nn.Linear(hid, dim).to(dev)
  with torch.no_grad():
    gru.weight_ih_l0.copy_(torch.from_numpy(params['gru_weight_ih'][0]))
    gru.weight_hh_l0.copy_(torch.from_numpy(params['gru_weight_hh'][0]))
    gru.bias_ih_l0.copy_(torch.from_numpy(params['gru_bias_ih'][0]))
    gru.bias_hh_l0.copy_(torch.from_numpy(params['gru_bias_hh'][0]))
    for lin, w, b in ((lin1, 'linear_mean1_weight', 'linear_mean1_bias'),
                      (lin2, 'linear_mean2_weight', 'linear_mean2_bias')):
      lin.weight.copy_(torch.from_numpy(params[w]))
      lin.bias.copy_(torch.from_numpy(params[b]))
  init_hidden = nn.Parameter(torch.zeros(1, 1, hid, device=dev))
  sigma2 = nn.Parameter(0.1 * torch.ones(dim, device=dev))
  rnn_params = list(gru.parameters()) + list(lin1.parameters()) + list(lin2.parameters())
  opt = torch.optim.Adam([{'params': rnn_params}, {'params': init_hidden}, {'params': sigma2}], lr=1e-3)
  padded = [torch.from_numpy(training.padded_batch(sub, b)).to(dev) for b in batches]
  lengths = [[len(sub[i]) + 1 for i in b] for b in batches]

  def step(x, lens):
    opt.zero_grad()
    packed = nn.utils.rnn.pack_padded_sequence(x, lens)
    out, _ = gru(packed, init_hidden.repeat(1, x.shape[1], 1))
    out, _ = nn.utils.rnn.pad_packed_sequence(out)
    mean = lin2(torch.relu(lin1(out)))
    mean = torch.cumsum(mean, dim=0) / torch.arange(1, mean.shape[0] + 1, device=dev).float().view(-1, 1, 1)
    truth = x[1:]
    diff2 = ((truth != 0).float() * mean[:-1] - truth) ** 2
    flat = diff2.view(-1, dim)
    n_d = (flat != 0).float().sum(dim=0)
    loss1 = (flat / (2 * sigma2)).sum() / (flat[:, 0] != 0).float().sum()
    loss2 = ((2 * 1.0 + n_d + 2) / (2 * n_d) * torch.log(sigma2)).sum() + (1.0 / (sigma2 * n_d)).sum()
    loss3 = 1e-5 * sum(torch.norm(p) for p in rnn_params)
    loss = loss1 + loss2 + loss3
    loss.backward()
    nn.utils.clip_grad_norm_(rnn_params, 5.0)
    opt.step()
    with torch.no_grad():
      sigma2.clamp_(min=1e-6)
    return loss

  for i in range(warmup):
    float(step(padded[i], lengths[i]))
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for i in range(warmup, len(batches)):
    last = float(step(padded[i], lengths[i]))   # .item(): one sync per iteration, like the HIP leg
  torch.cuda.synchronize()
  dt = time.perf_counter() - t0
  return {'ms_per_iter': 1e3 * dt / (len(batches) - warmup), 'last_loss': last,
          'torch': torch.__version__}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=200)
  ap.add_argument('--warmup', type=int, default=20)
  ap.add_argument('--utts', type=int, default=40)
  ap.add_argument('--frames', type=int, default=300)
  ap.add_argument('--no-torch', action='store_true')
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  params = weights.init_params(256, 512, 1, seed=0)
  sub, plan = data(a.utts, a.frames, 256)
  batches = [plan.next() for _ in range(a.warmup + a.iters)]
  T = [len(sub[b[0]]) + 1 for b in batches]
  res = {'recipe': {'utterances': a.utts, 'frames': a.frames, 'D': 256, 'H': 512, 'batch': 10,
                    'lr': 1e-3, 'iters': a.iters, 'warmup': a.warmup,
                    'T_mean': float(np.mean(T)), 'T_max': int(np.max(T)), 'sub_sequences': len(sub)},
         'design': 'launch-per-step recurrence (k_gru_fwd_step / k_gru_bwd_step), tiled FMA GEMMs',
         'hip': hip_leg(params, sub, batches, a.warmup)}
  if not a.no_torch:
    res['torch_rocm'] = torch_leg(params, sub, batches, a.warmup)
    res['speedup_vs_torch'] = res['torch_rocm']['ms_per_iter'] / res['hip']['ms_per_iter']
  line = json.dumps(res)
  print(line)
  if a.out:
    with open(a.out, 'w') as f:
      f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
  main()
