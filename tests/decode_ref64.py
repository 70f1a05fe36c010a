"""A float64 reference of the decode arithmetic that shares nothing with the product.

Plain numpy, written from the reference's formulas (uisrnn/uisrnn.py CoreRNN.forward and
_update_beam_state, uisrnn/loss_func.py weighted_mse_loss); it imports nothing of oracle/, include/ or
uisrnn_amd._capi and follows no canonical summation order (numpy's matrix product adds as it likes).

  step(params, x, h)               CoreRNN.forward of one row: mean, new hidden state, gate pre-activations
  weighted_mse(params, mean, x)    weighted_mse_loss with its dim-0 `nnz` quirk
  forced_nll(params, seq, labels)  neg_likelihood of a fixed trace from an empty beam state: total and per-frame
                                   losses (the meaning of forced_ref.score)
  Forced                           the same, one frame at a time (copy-on-write, for replaying a beam)

Next to every value it carries an A PRIORI bound on how far a float32 evaluation of the same formulas, in
any summation order, may lie from it (`*_bound`, `err` fields): computed from the float64 run alone, never
from what the code under test returns.  With u = 2^-24:

  dense chain of length K      (K + 16) (u (sum |w_k x_k| + |b|) + 2^-150)  +  sum |w_k| e(x_k)
  one +, -, *, /               u |result|  (+ 2^-150: a subnormal result)
  sigmoid, tanh                L e(argument) + 4 ulp(result) + 2^-125
                               L = the largest derivative over [argument - e, argument + e] (at most 1/4 and 1);
                               4 ulp: the 3.75 ulp measured for uis_tanhf, rounded up; 2^-125: what the clamps of
                               uis_expf at -87 / +88 may add where the true value is below the normal range
  r * gh_n                     |gh_n| e(r) + |r| e(gh_n)
  (a - b)^2 w, summed over D   2 |a - b| e(a) w per term, (D + 16) u sum |terms| for the additions

Two float32 decisions of the reference are float32 decisions here too, made on the float64 values rounded to
float32: whether (a_0 - b_0)^2 is zero (nnz; it underflows to zero below 2.6e-23), and whether a value is
beyond the float32 range (then it is +inf, as torch's float32 tensors have it).
"""

import math

import numpy as np

U = 2.0 ** -24
_TINY = 2.0 ** -150
_CLAMP = 2.0 ** -125
F32_MAX = float(np.finfo(np.float32).max)


def _f64(a):
  return np.asarray(a, dtype=np.float32).astype(np.float64)


def _rnd(v):
  """One correctly rounded float32 operation with result v."""
  return U * np.abs(v) + _TINY


def _ulp(v):
  return np.maximum(np.abs(v) * 2.0 ** -23, 2.0 ** -149)


def sigmoid(a):
  with np.errstate(over='ignore'):
    return np.where(a >= 0, 1.0 / (1.0 + np.exp(-np.abs(a))), np.exp(-np.abs(a)) / (1.0 + np.exp(-np.abs(a))))


def _sigmoid_err(a, e_a, s):
  t = sigmoid(np.maximum(np.abs(a) - e_a, 0.0))
  return t * (1.0 - t) * e_a + 4.0 * _ulp(s) + _CLAMP


def _tanh_err(a, e_a, n):
  t = np.tanh(np.maximum(np.abs(a) - e_a, 0.0))
  return (1.0 - t * t) * e_a + 4.0 * _ulp(n) + _CLAMP


def _dense(w, b, v, e_v):
  w, b = _f64(w), _f64(b)
  with np.errstate(over='ignore', invalid='ignore'):
    out = w @ v + b
    aw = np.abs(w)
    err = (w.shape[1] + 16) * (U * (aw @ np.abs(v) + np.abs(b)) + _TINY) + aw @ e_v
  return out, err


def step(params, x, h, e_h=None, with_err=False):
  """CoreRNN.forward of one row.  x [D], h [depth, H] (taken as float32 values).

  Returns (mean [D], h_out [depth, H], pre) in float64; pre[layer] = dict(r, z, n, gi_n, gh_n): the three gate
  pre-activations (n = gi_n + r * gh_n) and the two halves of the n gate's.  With with_err also
  (e_mean, e_h_out): the bound of the module docstring, e_h being the bound on the incoming hidden state."""
  with np.errstate(over='ignore', invalid='ignore', under='ignore'):   # (a bound may overflow; the caller checks the values)
    return _step(params, x, h, e_h, with_err)


def _step(params, x, h, e_h, with_err):
  """step() proper."""
  hid = int(params['rnn_hidden_size'])
  depth = int(params['rnn_depth'])
  inp = _f64(x).reshape(-1)
  e_inp = np.zeros_like(inp)
  h = np.asarray(h, dtype=np.float64).reshape(depth, hid)
  e_h = np.zeros_like(h) if e_h is None else np.asarray(e_h, dtype=np.float64).reshape(depth, hid)
  h_out = np.empty_like(h)
  e_out = np.empty_like(h)
  pre = []
  for l in range(depth):
    gi, e_gi = _dense(params['gru_weight_ih'][l], params['gru_bias_ih'][l], inp, e_inp)
    gh, e_gh = _dense(params['gru_weight_hh'][l], params['gru_bias_hh'][l], h[l], e_h[l])
    a_r = gi[:hid] + gh[:hid]
    a_z = gi[hid:2 * hid] + gh[hid:2 * hid]
    e_ar = e_gi[:hid] + e_gh[:hid] + _rnd(a_r)
    e_az = e_gi[hid:2 * hid] + e_gh[hid:2 * hid] + _rnd(a_z)
    r = sigmoid(a_r)
    z = sigmoid(a_z)
    e_r = _sigmoid_err(a_r, e_ar, r)
    e_z = _sigmoid_err(a_z, e_az, z)
    gi_n, gh_n = gi[2 * hid:], gh[2 * hid:]
    a_n = gi_n + r * gh_n
    e_an = (e_gi[2 * hid:] + np.abs(gh_n) * e_r + (r + e_r) * e_gh[2 * hid:] + _rnd(r * gh_n) + _rnd(a_n))
    n = np.tanh(a_n)
    e_n = _tanh_err(a_n, e_an, n)
    new = (1.0 - z) * n + z * h[l]
    t1 = h[l] - n
    e_new = (np.minimum(1.0 - z + e_z, 1.0) * e_n + np.minimum(z + e_z, 1.0) * e_h[l] + (np.abs(t1) + e_h[l] + e_n) * e_z +
             _rnd(t1) + _rnd(t1 * z) + _rnd(new))
    h_out[l], e_out[l] = new, e_new
    pre.append({'r': a_r, 'z': a_z, 'n': a_n, 'gi_n': gi_n, 'gh_n': gh_n})
    inp, e_inp = new, e_new
  y, e_y = _dense(params['linear_mean1_weight'], params['linear_mean1_bias'], inp, e_inp)
  y = np.maximum(y, 0.0)
  mean, e_mean = _dense(params['linear_mean2_weight'], params['linear_mean2_bias'], y, e_y)
  if with_err:
    return mean, h_out, pre, e_mean, e_out
  return mean, h_out, pre


def constants(params, with_err=False):
  """(m0, h1): the mean a new cluster is scored against and the hidden state it starts from --
  CoreRNN.forward of an all-zero frame from rnn_init_hidden (uisrnn.py:435-439)."""
  zero = np.zeros(int(params['observation_dim']), dtype=np.float32)
  mean, h1, _, e_mean, e_h1 = step(params, zero, _f64(params['rnn_init_hidden']), with_err=True)
  return (mean, h1, e_mean, e_h1) if with_err else (mean, h1)


def _to_f32_range(v):
  """float32's overflow: beyond its range a value is an infinity."""
  if v != v:
    return v
  if v > F32_MAX:
    return math.inf
  if v < -F32_MAX:
    return -math.inf
  return v


def weighted_mse(params, mean, x, e_mean=None, with_err=False):
  """weighted_mse_loss(mean, x, 1 / (2 sigma2)): mean(diff^2 w) * D * 1 / nnz, nnz = (diff_0^2 != 0)."""
  a = np.asarray(mean, dtype=np.float64).reshape(-1)
  b = _f64(x).reshape(-1)
  dim = a.shape[0]
  e_a = np.zeros(dim) if e_mean is None else np.asarray(e_mean, dtype=np.float64)
  w = 1.0 / (2.0 * _f64(params['sigma2']).reshape(-1))
  with np.errstate(over='ignore', invalid='ignore', under='ignore'):
    d = a - b
    terms = d * d * w
    total = float(np.mean(terms) * dim)
    e_d = e_a + _rnd(d)
    e_terms = w * ((2.0 * np.abs(d) + e_d) * e_d + _rnd(d * d)) + 5.0 * _rnd(terms)
    err = float(np.sum(e_terms) + (dim + 16) * U * np.sum(np.abs(terms)) + 3.0 * U * abs(total) + _TINY)
    d0 = np.float32(a[0]) - np.float32(b[0])
    nnz = 1.0 if np.float32(d0 * d0) != 0 else 0.0
    if nnz == 0.0:   # x / 0: +inf, or nan where the sum itself is zero
      total = math.inf if total > 0 else math.nan
  total = _to_f32_range(total)
  return (total, err) if with_err else total


class Forced:
  """The beam state of one hypothesis (uisrnn.py:55-78) under a trace given frame by frame."""

  def __init__(self, params, source=None):
    self.params = params
    if source is None:
      self.m0, self.h1, self.e_m0, self.e_h1 = constants(params, with_err=True)
      p0 = float(params['transition_bias'])
      self.lp_stay, self.lp_sw = math.log(1.0 - p0), math.log(p0)
      self.alpha = float(params['crp_alpha'])
      self.means, self.e_means, self.hids, self.e_hids, self.counts, self.blocks = [], [], [], [], [], []
      self.last, self.total, self.e_total, self.dead = -1, 0.0, 0.0, False
    else:
      for key in ('m0', 'h1', 'e_m0', 'e_h1', 'lp_stay', 'lp_sw', 'alpha', 'last', 'total', 'e_total', 'dead'):
        setattr(self, key, getattr(source, key))
      for key in ('means', 'e_means', 'hids', 'e_hids', 'counts', 'blocks'):
        setattr(self, key, list(getattr(source, key)))

  def advance(self, x, c):
    """A new state with frame x given to cluster c, the frame's loss and its bound."""
    new = Forced(self.params, self)
    c = int(c)
    k = len(new.means)
    if new.dead or c > k:     # the reference's invalid trace
      new.dead, new.total = True, math.inf
      return new, math.inf, 0.0
    sumblk = float(sum(new.blocks))
    if c < k:
      mse, e_mse = weighted_mse(new.params, new.means[c], x, new.e_means[c], with_err=True)
      if c == new.last:
        prior = new.lp_stay
      else:
        prior = new.lp_sw + math.log(new.blocks[c]) - math.log(sumblk + new.alpha)
      m, hid, _, e_m, e_hid = step(new.params, x, new.hids[c], new.e_hids[c], with_err=True)
      cnt = new.counts[c]    # frames of the trace in this cluster before this one
      with np.errstate(over='ignore', invalid='ignore'):
        scaled = new.means[c] * (cnt - 1.0)
        mean = (scaled + m) / cnt
        e_mean = (new.e_means[c] * (cnt - 1.0) + e_m + _rnd(scaled) + _rnd(scaled + m)) / cnt + _rnd(mean)
      new.means[c], new.e_means[c], new.hids[c], new.e_hids[c] = mean, e_mean, hid, e_hid
      new.counts[c] = cnt + 1
      if c != new.last:
        new.blocks[c] += 1
    else:
      mse, e_mse = weighted_mse(new.params, new.m0, x, new.e_m0, with_err=True)
      prior = new.lp_sw + math.log(new.alpha) - math.log(sumblk + new.alpha)
      m, hid, _, e_m, e_hid = step(new.params, x, new.h1, new.e_h1, with_err=True)
      new.means.append(m)
      new.e_means.append(e_m)
      new.hids.append(hid)
      new.e_hids.append(e_hid)
      new.counts.append(1)
      new.blocks.append(1)
    loss = _to_f32_range(mse - prior)
    e_loss = e_mse + U * abs(loss) + _TINY if math.isfinite(loss) else 0.0
    new.last = c
    new.total = _to_f32_range(new.total + loss)
    new.e_total = new.e_total + e_loss + (U * abs(new.total) if math.isfinite(new.total) else 0.0)
    return new, loss, e_loss


def forced_nll(params, seq, labels, with_err=False):
  """(total, per-frame losses [N]) of one utterance under `labels` (first-appearance form; a label beyond
  "one new cluster" makes the rest of the utterance +inf).  With with_err also their bounds."""
  x = np.asarray(seq, dtype=np.float32)
  state = Forced(params)
  losses = np.full(x.shape[0], np.inf)
  errs = np.zeros(x.shape[0])
  for t in range(x.shape[0]):
    state, losses[t], errs[t] = state.advance(x[t], labels[t])
    if state.dead:
      break
  if with_err:
    return state.total, losses, state.e_total, errs
  return state.total, losses
