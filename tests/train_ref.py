"""One training iteration of UIS-RNN in float64 (torch autograd and numpy, on the CPU).

What the trainer's tests compare uis_train.hip with:
  * dropout_scales   the trainer's inter-layer dropout multipliers, recomputed from its key
  * reference        losses, unclipped gradients in the trainer's flat order, per-tensor views of
                     them and the smallest live |pre-activation| of linear_mean1 (the ReLU kink)
  * torch_gradients  reference()'s flat gradient and losses alone
  * clip             clip_grad_norm_ over the CoreRNN segments
  * adam_replay      Adam over a given sequence of gradients, with the sigma2 clamp
tests/test_train_ref_host.py ties all of it to the reference's recorded fit().
"""

import collections

import numpy as np

M64 = (1 << 64) - 1

_PER_LAYER = ('gru_weight_ih', 'gru_weight_hh', 'gru_bias_ih', 'gru_bias_hh')
_TAIL = ('linear_mean1_weight', 'linear_mean1_bias', 'linear_mean2_weight', 'linear_mean2_bias',
         'rnn_init_hidden', 'sigma2')


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


def segments(dim, hidden, depth):
  """(name, flat slice, 2-D shape) of every tensor in the trainer's flat order; a vector is [1, n]."""
  shapes = []
  for l in range(depth):
    shapes += [('gru_weight_ih[{}]'.format(l), (3 * hidden, dim if l == 0 else hidden)),
               ('gru_weight_hh[{}]'.format(l), (3 * hidden, hidden)),
               ('gru_bias_ih[{}]'.format(l), (1, 3 * hidden)),
               ('gru_bias_hh[{}]'.format(l), (1, 3 * hidden))]
  shapes += [('linear_mean1_weight', (hidden, hidden)), ('linear_mean1_bias', (1, hidden)),
             ('linear_mean2_weight', (dim, hidden)), ('linear_mean2_bias', (1, dim)),
             ('rnn_init_hidden', (depth, hidden)), ('sigma2', (1, dim))]
  out, pos = [], 0
  for name, shape in shapes:
    out.append((name, slice(pos, pos + shape[0] * shape[1]), shape))
    pos += shape[0] * shape[1]
  return out


def n_rnn(dim, hidden, depth):
  """The length of the CoreRNN part of the flat vector (what clip_grad_norm_ and loss3 cover)."""
  return segments(dim, hidden, depth)[-2][1].start


def flatten(params):
  """The flat float64 vector of a parameter dict."""
  parts = [np.asarray(params[key][l], np.float64).ravel()
           for l in range(int(params['rnn_depth'])) for key in _PER_LAYER]
  parts += [np.asarray(params[key], np.float64).ravel() for key in _TAIL]
  return np.concatenate(parts)


def unflatten(flat, dim, hidden, depth):
  """A float64 parameter dict from a flat vector (uisrnn_amd._capi.unflatten_params rounds to float32)."""
  flat = np.asarray(flat, np.float64)
  out = {'observation_dim': dim, 'rnn_hidden_size': hidden, 'rnn_depth': depth}
  for key in _PER_LAYER:
    out[key] = [None] * depth
  for name, sl, shape in segments(dim, hidden, depth):
    value = flat[sl].reshape(shape)
    if name.startswith('gru_'):
      key, l = name[:-1].split('[')
      out[key][int(l)] = value if 'weight' in key else value.ravel()
    elif name in ('linear_mean1_weight', 'linear_mean2_weight', 'rnn_init_hidden'):
      out[name] = value
    else:
      out[name] = value.ravel()
  return out


Reference = collections.namedtuple('Reference', 'flat losses segments min_preact')


def reference(params, padded, lengths, masks, reg=1e-5, alpha=1.0, beta=1.0):
  """One iteration of the reference's loss in float64 torch (CPU), the given dropout masks between
  layers, no clipping.

  flat        the gradient in the trainer's flat order
  losses      [loss, loss1, loss2, loss3]
  segments    segments(): (name, slice, 2-D shape) per tensor, to cut views of `flat`
  min_preact  the smallest |linear_mean1 pre-activation| over the rows (t, b) with t < lengths[b]:
              how far the iteration stays from ReLU's kink, where the gradient jumps
  """
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
    if l > 0 and masks and masks.get(l) is not None:  # no mask: no dropout before this layer
      seq = seq * t64(masks[l]).view(seq.shape)
    packed = nn.utils.rnn.pack_padded_sequence(seq, lengths)
    out, _ = gru(packed, h0[l:l + 1].repeat(1, x.shape[1], 1))
    seq, _ = nn.utils.rnn.pad_packed_sequence(out, total_length=x.shape[0])
  pre = lin1(seq)
  live = torch.arange(x.shape[0]).view(-1, 1) < torch.tensor([int(n) for n in lengths]).view(1, -1)
  min_preact = float(pre.detach().abs()[live].min())
  mean = lin2(torch.relu(pre))
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
  return Reference(np.concatenate(grads), [float(v.detach()) for v in losses], segments(dim, hid, depth),
                   min_preact)


def torch_gradients(params, padded, lengths, masks, reg=1e-5, alpha=1.0, beta=1.0):
  """reference()'s flat gradient and losses."""
  ref = reference(params, padded, lengths, masks, reg, alpha, beta)
  return ref.flat, ref.losses


def clip_coefficient(flat, n_rnn, max_norm):  # pylint: disable=redefined-outer-name
  """torch's clip_grad_norm_ factor for the CoreRNN part flat[:n_rnn]: max_norm / (norm + 1e-6), at most 1."""
  norm = np.linalg.norm(np.asarray(flat[:n_rnn], np.float64))
  return min(float(max_norm) / (norm + 1e-6), 1.0)


def clip(flat, n_rnn, max_norm):  # pylint: disable=redefined-outer-name
  """The gradient after clip_grad_norm_ over flat[:n_rnn]; what follows (rnn_init_hidden, sigma2) is kept."""
  out = np.array(flat, dtype=np.float64)
  out[:n_rnn] *= clip_coefficient(out, n_rnn, max_norm)
  return out


def adam_replay(p0, grads_per_step, lr, n_adam, sigma_slice):
  """torch.optim.Adam (betas 0.9 / 0.999, eps 1e-8) from p0 over the given gradients, in float64.

  The bias correction is k_clip_adam's and torch's: p -= lr / (1 - 0.9^k) · m / (sqrt(v) / sqrt(1 - 0.999^k) + eps).
  After each step the sigma slice is clamped at 1e-6; elements at or past n_adam are never touched.
  Returns the parameters after every step."""
  p = np.array(p0, dtype=np.float64)
  m = np.zeros(n_adam)
  v = np.zeros(n_adam)
  out = []
  for k, g in enumerate(grads_per_step, 1):
    g = np.asarray(g, np.float64)[:n_adam]
    m = 0.9 * m + 0.1 * g
    v = 0.999 * v + 0.001 * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - 0.999 ** k) + 1e-8
    p[:n_adam] -= lr / (1.0 - 0.9 ** k) * (m / denom)
    p[sigma_slice] = np.maximum(p[sigma_slice], 1e-6)
    out.append(p.copy())
  return out
