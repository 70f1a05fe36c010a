"""Hostile numerics for the decode path: models and utterances that drive the step into the territory
benign data never reaches -- the clamps of uis_expf, the |x| <= 0.5 switch of uis_tanhf, subnormal operands
and results, overflowing and vanishing weighted MSEs.

Every regime builds a Case (params, seqs) from fixed seeds and has a `reached` check, computed on the CPU
from tests/decode_ref64.py or the oracle and never from a device output, that fails when the regime has
silently turned benign.  A test calls reached() before it looks at anything the device returned.

  edges         all GRU weights zero: every r / z pre-activation is exactly b_ih + b_hh, the n gate sees
                b_in + r * b_hn (b_hn = 0 on four units of five: there tanh gets the edge itself); the biases walk
                EDGES over the units; rnn_init_hidden is not zero
  saturated40   natural U(+-1/sqrt(H)) weights, the GRU matrices x 40 (frames x 8 or more so that the gates leave +-88)
  saturated200  ... x 200
  subnormal     frames with features in 1e-45 .. 1e-38, -0.0 and exact zeros; linear_mean2_bias and bands of
                W_ih subnormal; one hidden unit that is subnormal end to end decides, through dim 0 of the
                mean and the nnz quirk of the weighted MSE, whether ANY candidate is finite
  overflow      frames with features of 1e18 .. 1e20 at sigma2 0.1: finite, 3.2e38 (every later score ties),
                and +inf candidates in one batch
  sigma_small   sigma2 1e-6: scores around 1e7 .. 1e8; linear_mean2_weight x 2^-24, so that the cluster means
                differ less than the rounding of the running score: masses of exact ties for the index tie-break
  sigma_large   sigma2 1e+6: the MSE vanishes against the prior; transition_bias 0.9 opens clusters
"""

import collections

import numpy as np

import decode_ref64
from uisrnn_amd import weights

REGIMES = ('edges', 'saturated40', 'saturated200', 'subnormal', 'overflow', 'sigma_small', 'sigma_large')

Case = collections.namedtuple('Case', 'regime params seqs info')

_F32 = np.float32


def _around(v, steps=(-2, -1, 0, 1, 2)):
  """v and its float32 neighbours on either side."""
  out = []
  for s in steps:
    x = _F32(v)
    for _ in range(abs(s)):
      x = np.nextafter(x, _F32(np.inf) if s > 0 else _F32(-np.inf))
    out.append(x)
  return out


def _edge_list():
  vals = []
  for base in (0.5, 87.0, 88.0, 88.5, 100.0, 1e30, 1e-40, 16.65, 0.4938):   # (nextafter(0.5) is among 0.5's neighbours)
    for sign in (1.0, -1.0):
      vals += _around(sign * base)
  vals += [_F32(0.0), _F32(-0.0)] + _around(0.0, (-2, -1, 1, 2))
  # tanh(+-0.5) has the same bits on either side of uis_tanhf's switch (0x1.d9353ep-2 from the series and from the exp
  # form), and so have 0.4938 and its neighbours: a moved switch shows only where the two forms differ.  The nearest
  # such points, with both float32 neighbours on each side differing too: 7 ulp below 0.5 and 15 ulp above it.
  for base in (float.fromhex('0x1.fffff2p-2'), float.fromhex('0x1.00001ep-1')):
    for sign in (1.0, -1.0):
      vals += _around(sign * base)
  return np.array(vals, dtype=np.float32)


EDGES = _edge_list()   # 116 values
# What a pre-activation can be: every dense chain ends by adding its +0.0 segments (include/uis_numerics.h), so the
# -0.0 entry arrives at the gate as +0.0.
EDGES_SEEN = EDGES + _F32(0.0)
B_HN_PERIOD = 5        # b_hn is 0.75 on every fifth unit: coprime with len(EDGES), so every edge also meets b_hn = 0


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _frames(rng, lengths, dim):
  cents = rng.standard_normal((3, dim))
  return [cents[np.repeat(rng.integers(0, 3, size=n // 4 + 1), 4)[:n]] * 0.4 + 0.1 * rng.standard_normal((n, dim))
          for n in lengths]


def _natural(dim, hidden, depth, seed, sigma2=0.1, transition_bias=0.2):
  params = weights.init_params(dim, hidden, depth, sigma2=sigma2, transition_bias=transition_bias, crp_alpha=1.0,
                               seed=seed)
  params['rnn_init_hidden'] = (0.2 * np.random.default_rng(seed + 1).standard_normal((depth, hidden))).astype(np.float32)
  return params


def edge_slices(hidden, depth, offset):
  """Which EDGES entry gate g (r, z, n) of layer l gives unit j: [depth, 3, hidden] indices."""
  unit = np.arange(hidden)[None, None, :]
  gate = np.arange(3)[None, :, None]          # n runs 64 entries ahead of r: +-0.0 meets r = sigmoid(-88)
  layer = np.arange(depth)[:, None, None]
  return (unit + 32 * gate + 7 * layer + offset) % len(EDGES)


def _edges(params, offset):
  hid, depth = params['rnn_hidden_size'], params['rnn_depth']
  sl = edge_slices(hid, depth, offset)
  for l in range(depth):
    params['gru_weight_ih'][l] = np.zeros_like(params['gru_weight_ih'][l])
    params['gru_weight_hh'][l] = np.zeros_like(params['gru_weight_hh'][l])
    b_ih = np.zeros(3 * hid, dtype=np.float32)
    b_hh = np.zeros(3 * hid, dtype=np.float32)
    unit = np.arange(hid)
    for g in range(2):           # r, z: the edge value on one side, an exact zero on the other
      v = EDGES[sl[l, g]]
      b_ih[g * hid:(g + 1) * hid] = np.where(unit % 2 == 0, v, _F32(0.0))
      b_hh[g * hid:(g + 1) * hid] = np.where(unit % 2 == 0, _F32(0.0), v)
    b_ih[2 * hid:] = EDGES[sl[l, 2]]                                  # n: gi_n is the edge value ...
    b_hh[2 * hid:] = np.where((unit + offset) % B_HN_PERIOD == 0, _F32(0.75), _F32(0.0))   # ... plus r * 0.75 on one unit of five
    params['gru_bias_ih'][l], params['gru_bias_hh'][l] = b_ih, b_hh
  return {'offset': offset}


def _subnormals(rng, shape):
  """Random float32 subnormals of either sign, 2^-149 .. 2^-127."""
  mag = rng.integers(1, 1 << 22, size=shape).astype(np.uint32) >> rng.integers(0, 22, size=shape).astype(np.uint32)
  mag = np.maximum(mag, 1).astype(np.uint32)
  sign = (rng.integers(0, 2, size=shape).astype(np.uint32) << np.uint32(31))
  return (mag | sign).view(np.float32)


def _subnormal(params, seqs, rng):
  hid, depth, dim = params['rnn_hidden_size'], params['rnn_depth'], params['observation_dim']
  top = depth - 1
  j0, i0, i1 = hid - 1, hid - 2, hid - 3
  for l in range(depth):     # a band of W_ih: the n-gate rows of the last hidden units
    band = params['gru_weight_ih'][l][2 * hid + hid - 2:3 * hid]
    band[...] = _subnormals(rng, band.shape)
  # unit j0 of the top layer: n = tanh(subnormal . input), nothing else feeds it
  params['gru_weight_hh'][top][2 * hid + j0] = 0.0
  params['gru_bias_ih'][top][2 * hid + j0] = 0.0
  params['gru_bias_hh'][top][2 * hid + j0] = 0.0
  params['rnn_init_hidden'][top, j0] = _F32(3e-39)
  # linear_mean1 rows i0, i1 = +-h[j0]; dim 0 of the mean = 2^56 |h[j0]| + a subnormal bias: about 1e-22
  w1, b1, w2 = params['linear_mean1_weight'], params['linear_mean1_bias'], params['linear_mean2_weight']
  w1[i0], w1[i1] = 0.0, 0.0
  w1[i0, j0], w1[i1, j0] = 1.0, -1.0
  b1[i0], b1[i1] = 0.0, 0.0
  w2[0] = 0.0
  w2[0, i0], w2[0, i1] = 2.0 ** 56, 2.0 ** 56
  params['linear_mean2_bias'] = _subnormals(rng, (dim,))
  tiny = np.array([0.0, -0.0, 1e-45, -3e-42, 1e-40, 1e-38, -7e-39], dtype=np.float32)
  out = []
  for s in seqs:
    s = np.asarray(s, dtype=np.float32)
    mask = rng.random(s.shape) < 0.15
    s[mask] = tiny[rng.integers(0, len(tiny), size=int(mask.sum()))]
    s[:, 0] = tiny[(np.arange(s.shape[0]) + len(out)) % len(tiny)]   # dim 0: (mean_0 - x_0)^2 is subnormal, never zero
    out.append(s.astype(np.float64))
  return out, {'j0': j0}


def _overflow(seqs):
  out = []
  for u, s in enumerate(seqs):
    s = np.array(s, dtype=np.float64)
    n = s.shape[0]
    kind = u % 4
    if kind == 0:      # 1e18: a term of 5e36, finite however many there are in an utterance this short
      s[2, 3], s[n // 2, 7], s[n - 1, 3] = 1e18, -1e18, 2e18
    elif kind == 1:    # one frame of 3.2e38: every later loss is absorbed, all hypotheses tie
      s[n // 2, 3] = 8e18
    elif kind == 2:    # the square itself overflows: every candidate of that frame is +inf
      s[5, 3] = 1e20
    else:              # 3.2e38 twice: the running score overflows at the second
      s[3, 3], s[n - 2, 5] = 8e18, -8e18
    out.append(s)
  return out


def build(regime, dim, hidden, depth=1, lengths=(12, 9, 15, 8), seed=0, offset=0):
  """The Case of `regime` at a model shape.  `offset` rotates EDGES over the units (edges only)."""
  assert regime in REGIMES, regime
  rng = np.random.default_rng(1000 * seed + 17 * dim + hidden + REGIMES.index(regime))
  sigma2 = {'sigma_small': 1e-6, 'sigma_large': 1e6}.get(regime, 0.1)
  params = _natural(dim, hidden, depth, seed + 31 * REGIMES.index(regime), sigma2=sigma2,
                    transition_bias=0.9 if regime == 'sigma_large' else 0.2)
  seqs = _frames(rng, lengths, dim)
  info = {}
  if regime == 'edges':
    info = _edges(params, offset)
  elif regime in ('saturated40', 'saturated200'):
    gain = 40.0 if regime == 'saturated40' else 200.0
    for l in range(depth):
      params['gru_weight_ih'][l] = params['gru_weight_ih'][l] * _F32(gain)
      params['gru_weight_hh'][l] = params['gru_weight_hh'][l] * _F32(gain)
    if gain == 40.0:   # W_ih x as wide as W_hh h: about 60 a pre-activation
      seqs = [s * max(8.0, 12.0 * (hidden / (2.0 * dim)) ** 0.5) for s in seqs]
  elif regime == 'subnormal':
    seqs, info = _subnormal(params, seqs, rng)
  elif regime == 'overflow':
    seqs = _overflow(seqs)
  elif regime == 'sigma_small':
    # cluster means 2^-24 apart: the candidates of a step differ by less than an ulp of the running score
    params['linear_mean2_weight'] = params['linear_mean2_weight'] * _F32(2.0 ** -24)
  return Case(regime, params, seqs, info)


def is_subnormal(a):
  a = np.abs(np.asarray(a, dtype=np.float64))
  return (a > 0) & (a < 2.0 ** -126)


def zero_subnormals(case):
  """The same data with every subnormal parameter and feature replaced by zero."""
  def flush(a):
    a = np.array(a, dtype=np.float32)
    a[is_subnormal(a)] = 0.0
    return a
  params = dict(case.params)
  for key, val in case.params.items():
    if isinstance(val, list):
      params[key] = [flush(v) for v in val]
    elif isinstance(val, np.ndarray) and val.dtype == np.float32:
      params[key] = flush(val)
  return Case(case.regime, params, [flush(s).astype(np.float64) for s in case.seqs], case.info)


def chain_preacts(case, utterance=0):
  """Gate pre-activations (float64, decode_ref64) along utterance `utterance` held in ONE cluster, plus those of
  the new-cluster constant: dict r, z, n, gi_n -> [steps, depth, H], and the z gate values."""
  params = case.params
  acc = {k: [] for k in ('r', 'z', 'n', 'gi_n')}
  h = np.asarray(params['rnn_init_hidden'], dtype=np.float64)
  xs = [np.zeros(params['observation_dim'], dtype=np.float32)] + list(np.asarray(case.seqs[utterance], dtype=np.float32))
  for x in xs:
    _, h, pre = decode_ref64.step(params, x, h)
    for k in acc:
      acc[k].append(np.stack([p[k] for p in pre]))
  return {k: np.stack(v) for k, v in acc.items()}


def gate_arguments(case, pre=None):
  """The float32 bit patterns the r gate's sigmoid, the z gate's sigmoid and the n gate's tanh are given along
  chain_preacts(case): three sets."""
  pre = chain_preacts(case) if pre is None else pre
  return [set(_bits(pre[k]).ravel().tolist()) for k in ('r', 'z', 'n')]


def reached(case, oracle, ref=None, beam=None):
  """Fail unless `case` is in its regime.  `ref` = the oracle's decode of the case (look_ahead 1,
  test_iteration 1) at beam size `beam`: needed by subnormal, overflow and the sigma regimes."""
  regime, params = case.regime, case.params
  hid, depth = params['rnn_hidden_size'], params['rnn_depth']
  if regime == 'edges':
    pre = chain_preacts(case)
    sl = edge_slices(hid, depth, case.info['offset'])
    want = _bits(EDGES_SEEN[sl])                             # [depth, 3, hid]
    plain = np.broadcast_to(((np.arange(hid) + case.info['offset']) % B_HN_PERIOD != 0)[None, :], (depth, hid))
    for t in range(pre['r'].shape[0]):                       # exactly the edge values, in bits, at every step
      assert np.array_equal(_bits(pre['r'][t]), want[:, 0]) and np.array_equal(_bits(pre['z'][t]), want[:, 1])
      assert np.array_equal(_bits(pre['gi_n'][t]), want[:, 2])
      assert np.array_equal(_bits(pre['n'][t])[plain], want[:, 2][plain])     # what tanh is given where b_hn = 0
    if hid >= len(EDGES):                                    # every edge reaches sigmoid twice over and tanh
      for seen in gate_arguments(case, pre):
        assert set(_bits(EDGES_SEEN).tolist()) <= seen
    assert np.any(np.asarray(params['rnn_init_hidden']) != 0)
    r_edge, n_edge = EDGES[sl[:, 0]], EDGES[sl[:, 2]]
    meets = (r_edge < -87.4) & (n_edge == 0) & ~plain
    assert meets.any() or hid < B_HN_PERIOD * len(EDGES)
    if meets.any():                                          # r (subnormal) * b_hn, added to a zero b_in
      assert np.all(is_subnormal(pre['n'][:, meets]))
  elif regime in ('saturated40', 'saturated200'):
    pre = chain_preacts(case)
    rz = np.concatenate([pre['r'].ravel(), pre['z'].ravel()])
    frac = float(np.mean(np.abs(rz) > 88.0))
    assert frac >= 0.05, frac
    assert np.any(is_subnormal(decode_ref64.sigmoid(pre['z']))), 'no subnormal z gate'
  elif regime == 'subnormal':
    assert any(np.any(is_subnormal(np.asarray(s, dtype=np.float32))) for s in case.seqs)
    assert any(np.any(np.signbit(np.asarray(s)) & (np.asarray(s) == 0)) for s in case.seqs)
    assert np.all(is_subnormal(params['linear_mean2_bias']))
    assert all(np.any(is_subnormal(w)) for w in params['gru_weight_ih'])
    pre = chain_preacts(case)
    assert np.all(is_subnormal(pre['n'][1:, depth - 1, case.info['j0']]) | (np.abs(pre['n'][1:, depth - 1, case.info['j0']]) < 1e-36))
    assert np.any(is_subnormal(pre['n'][1:, depth - 1, case.info['j0']]))     # subnormal products, summed
    flushed = zero_subnormals(case)
    other = oracle.decode(flushed.params, flushed.seqs, beam, 1, 1, n_threads=8)
    differ = (not all(np.array_equal(a, b) for a, b in zip(ref['labels'], other['labels'])) or
              not np.array_equal(_bits(ref['scores']), _bits(other['scores'])))
    assert differ, 'zeroing the subnormals changes nothing: a flush would be invisible'
    assert any((l >= 0).all() for l in ref['labels'])
  elif regime == 'overflow':
    scores = ref['beam_scores']
    assert np.isposinf(scores).any() and np.isfinite(scores).any()
    assert np.isposinf(ref['scores']).any() and np.isfinite(ref['scores']).any()
    assert any((l >= 0).all() for l in ref['labels']) and any((l == -1).all() for l in ref['labels'])
    assert (ref['scores'][np.isfinite(ref['scores'])] > 1e38).any()      # the 3.2e38 utterance stayed alive
  elif regime == 'sigma_small':
    ties = sum(len(np.unique(_bits(row[np.isfinite(row)]))) < int(np.isfinite(row).sum()) for row in ref['beam_scores'])
    assert ties >= max(1, len(ref['beam_scores']) // 2), 'exact ties in fewer than half of the final beams'
    assert float(np.min(ref['scores'])) > 5e6
  elif regime == 'sigma_large':
    assert int(ref['max_clusters'].max()) >= 2
    assert float(np.max(np.abs(ref['scores']))) < 1e3
  return True


# ---- the comparisons the host and the GPU tests share

# (observation_dim, hidden, depth): the model shapes of the decode kernel families (tests/test_gpu_hostile.py)
SHAPES = ((256, 512, 1), (128, 256, 1), (72, 300, 1), (512, 512, 1), (48, 256, 2), (16, 8, 1), (33, 17, 2))


def worst_ratio(got, want, err):
  """max |got - want| / err over the finite entries; where `want` is not finite `got` must be the same
  infinity, or a nan too."""
  got = np.asarray(got, dtype=np.float64).ravel()
  want = np.asarray(want, dtype=np.float64).ravel()
  err = np.asarray(err, dtype=np.float64).ravel() if np.ndim(err) else np.full(want.shape, float(err))
  assert got.shape == want.shape == err.shape
  fin = np.isfinite(want)
  assert np.array_equal(np.isnan(got), np.isnan(want)), 'nan in different places'
  assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), 'infinities differ'
  assert np.all(np.isfinite(got[fin])), 'not finite where the float64 reference is'
  if not fin.any():
    return 0.0
  return float(np.max(np.abs(got[fin] - want[fin]) / err[fin]))


def step_rows(case, oracle, n_rows=6):
  """(x, h) rows for rnn_step: the new-cluster constant, then utterance 0 along one cluster, the hidden state
  being the oracle's float32 one."""
  params = case.params
  x = np.zeros(params['observation_dim'], dtype=np.float32)
  h = np.asarray(params['rnn_init_hidden'], dtype=np.float32)
  rows = []
  for t in range(n_rows):
    rows.append((x, h))
    _, h = oracle.rnn_step(params, x, h)
    x = np.asarray(case.seqs[0][t], dtype=np.float32)
  return rows


def check_step(case, rows, step_fn):
  """step_fn(x, h) -> (mean, h_out) in float32 against decode_ref64.step and its bound; the worst ratio."""
  worst = 0.0
  for x, h in rows:
    mean, hout = step_fn(x, h)
    m64, h64, _, e_m, e_h = decode_ref64.step(case.params, x, h, with_err=True)
    worst = max(worst, worst_ratio(mean, m64, e_m), worst_ratio(hout, h64, e_h))
  assert worst <= 1.0, worst
  return worst


def labelings(case, ref):
  """The oracle's labels (all zeros for an utterance whose beam died) and an alternating labeling."""
  own = [np.where(l < 0, 0, l).astype(np.int32) for l in ref['labels']]
  alt = [np.arange(len(s), dtype=np.int32) % 2 for s in case.seqs]
  return {'oracle': own, 'alternating': alt}


def check_forced(case, labels, scores, losses, utterances=None):
  """float32 totals and per-frame losses (lists per utterance) against decode_ref64.forced_nll and its bound.

  Along a trace the bound is pushed through |W_hh| at every step and, with the GRU matrices x 40 / x 200, passes
  the values themselves after a few frames; a comparison against such a bound proves nothing.  So a frame (a
  total) is compared only where its bound is at most half the value -- non-finite values always are.
  Returns (worst ratio, frames compared, frames); the caller asserts that frames were compared."""
  worst, used, seen = 0.0, 0, 0
  for u in (range(len(case.seqs)) if utterances is None else utterances):
    total, per, e_total, e_per = decode_ref64.forced_nll(case.params, case.seqs[u], labels[u], with_err=True)
    bites = ~np.isfinite(per) | (e_per <= 0.5 * np.abs(per))
    worst = max(worst, worst_ratio(np.asarray(losses[u])[bites], per[bites], e_per[bites]))
    if not np.isfinite(total) or e_total <= 0.5 * abs(total):
      worst = max(worst, worst_ratio([scores[u]], [total], e_total))
    used, seen = used + int(bites.sum()), seen + len(per)
  assert worst <= 1.0, worst
  return worst, used, seen


# (observation_dim, hidden, depth, offset) of the edges cases on the k_decode_small shapes: hidden sizes below
# len(EDGES) see a slice of the list per gate; between them these give every gate every edge (tests/test_ref64_host.py)
SMALL_EDGE_CASES = tuple((16, 8, 1, o) for o in range(0, 116, 4)) + tuple((33, 17, 2, o) for o in range(0, 116, 13))
