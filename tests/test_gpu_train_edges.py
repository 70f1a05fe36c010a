"""uis_train.hip against float64 autograd (tests/train_ref.py) at its tile and chunk edges.

_capi.Trainer directly (set_data, step, flat_grads): train()'s host preparation is not involved.

Gradients and losses, five shapes (lengths are the reference's seq_lengths, rows + 1):
  A  D 3 / H 1025, lengths 5, 3          k_gru_fwd_step's second LDS chunk (one element), five unit
                                         blocks (the last holds one unit), k_gru_bwd_step with four
                                         chunks (the last holds 3), 770 norm partials (> 256), GEMM N 3075
  B  D 65 / H 65 / depth 2, 4, 4, 2      every GEMM extent one past a tile (N 195 and 65, K 65 and 12,
                                         M 12), k_colsum at 65 and 195 columns, the depth-2 dX GEMM
  C  D 17 / H 300, length 2              B = 1, T = 2, k_colsum over 2 rows, a partial second unit block
  D  D 70 / H 342, 11 ragged columns     3H = 1026, T·B = 99 (two M tiles), ties among the lengths
  E  D 5 / H 24 / depth 2, 5 columns     exact zeros in the observations (one entry of dimension 0, one
                                         whole row, one whole dimension of a column): the truth != 0
                                         mask, n_d and nz all move; at dropout 0 and 0.4
Each asserts the four losses within 1e-5 relative, every tensor's gradient within TOL norm-relative
(‖dev − ref‖ / ‖ref‖), and by the same measure every slice of a tensor that lies in the last 64-wide
tile of its rows, of its columns, or of both, and in the last 256-wide block of an H-long axis (per
gate where the axis is 3H long): one wrong column barely moves the norm of a 3-million-element tensor.
TOL = 1e-5: float32 against float64 CPU autograd differs by 1e-7 .. 1.1e-6 per tensor and slice on these
cases; ten times that allows for the kernels' own (fixed) summation order.  The comparison only means
something away from ReLU's kink, so each test first asserts that the reference's smallest live
|linear_mean1 pre-activation| is >= 1e-5; the data seeds were picked on the CPU for that.

Then, on shapes B and E: the clip coefficient and what it leaves alone, Adam's arithmetic against a
float64 replay of the device's own gradients, the sigma2 >= 1e-6 clamp, estimate_sigma2=False, one
trainer reused across batches of changing (B, T), and argument errors.
"""

import functools

import numpy as np
import pytest

import train_ref
from uisrnn_amd import _capi
from uisrnn_amd import training
from uisrnn_amd import weights

pytestmark = pytest.mark.gpu

TOL = 1e-5
MIN_PREACT = 1e-5
KEY = 0x0123456789abcdef

# name: (D, H, depth, lengths, data seed)
SHAPES = {
    'A': (3, 1025, 1, (5, 3), 11),
    'B': (65, 65, 2, (4, 4, 2), 8),
    'C': (17, 300, 1, (2,), 6),
    'D': (70, 342, 1, (9, 9, 8, 7, 7, 6, 4, 3, 2, 2, 2), 38),
    'E': (5, 24, 2, (12, 9, 9, 4, 2), 1),
}
# further sub-sequences behind E's five, for the batches of test_one_trainer_across_batch_shapes
EXTRA_LENGTHS = (3, 3, 2)


@functools.lru_cache(maxsize=None)
def make_case(name, seed=None, scale=None):
  """(params, sub-sequences) of a shape: init_params weights, rnn_init_hidden 0.1·N(0,1), sigma2 in
  [0.05, 0.25], N(0,1) rows (times `scale` per dimension), E's zeros.  Cached: treat as read-only."""
  dim, hidden, depth, lengths, default_seed = SHAPES[name]
  seed = default_seed if seed is None else seed
  params = weights.init_params(dim, hidden, depth, transition_bias=0.5, seed=seed)
  rng = np.random.RandomState(seed)
  params['rnn_init_hidden'] = (0.1 * rng.randn(depth, hidden)).astype(np.float32)
  params['sigma2'] = rng.uniform(0.05, 0.25, dim).astype(np.float32)
  if name == 'E':
    lengths = lengths + EXTRA_LENGTHS
  sub = [rng.randn(n - 1, dim).astype(np.float32) for n in lengths]
  if scale is not None:
    sub = [s * np.asarray(scale, np.float32) for s in sub]
  if name == 'E':
    sub[0][3, 0] = 0.0   # one entry of dimension 0: nz and n_0 drop by one
    sub[1][2, :] = 0.0   # a whole row: every n_d drops
    sub[2][:, 3] = 0.0   # dimension 3 of a whole column
  return params, sub


def batch_of(name):
  return list(range(len(SHAPES[name][3])))


@functools.lru_cache(maxsize=None)
def reference_of(name, dropout=0.0, seed=None):
  """The float64 iteration 0 of a shape's batch (shared by the tests; read-only)."""
  params, sub = make_case(name, seed)
  dim, hidden, depth, _, _ = SHAPES[name]
  idx = batch_of(name)
  padded = training.padded_batch(sub, idx)
  lengths = [len(sub[i]) + 1 for i in idx]
  masks = {}
  for l in range(1, depth):
    masks[l] = train_ref.dropout_scales(KEY, 0, l, padded.shape[0] * padded.shape[1] * hidden, dropout)
  return train_ref.reference(params, padded, lengths, masks)


def _rel(a, b):
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def edge_slices(shape, hidden):
  """(label, row slice, column slice) of a [rows, cols] tensor's edges: the last 64-wide tile of each
  axis (rows 64·⌊(M−1)/64⌋:, columns likewise) and the last 256-wide block of each H-long run of an
  axis of H or 3H, alone and combined with each other; the whole tensor is not among them."""
  def axis(n):
    out = [('all', slice(0, n))]
    if n > 1:
      out.append(('last tile', slice(64 * ((n - 1) // 64), n)))
      if n in (hidden, 3 * hidden):
        for g in range(n // hidden):
          out.append(('block of run {}'.format(g), slice(g * hidden + 256 * ((hidden - 1) // 256), (g + 1) * hidden)))
    return out
  seen, out = {(0, shape[0], 0, shape[1])}, []
  for rl, rs in axis(shape[0]):
    for cl, cs in axis(shape[1]):
      key = (rs.start, rs.stop, cs.start, cs.stop)
      if key not in seen:
        seen.add(key)
        out.append(('rows {} x cols {} [{}:{}, {}:{}]'.format(rl, cl, *key), rs, cs))
  return out


def compare(name, losses, grads, ref, hidden):
  """Print the case's worst figures, then assert losses, tensors and edge slices."""
  loss_err = [abs(a - b) / abs(b) for a, b in zip(losses, ref.losses)]
  tensors, slices = [], []
  for seg_name, sl, shape in ref.segments:
    dev2, ref2 = grads[sl].reshape(shape), ref.flat[sl].reshape(shape)
    tensors.append((_rel(dev2, ref2), seg_name))
    for label, rs, cs in edge_slices(shape, hidden):
      slices.append((_rel(dev2[rs, cs], ref2[rs, cs]), '{} {}'.format(seg_name, label)))
  print('\ncase {}: min |pre-activation| {:.2e}; worst loss {:.2e}; worst tensor {:.2e} ({}); '
        'worst of {} edge slices {:.2e} ({})'.format(name, ref.min_preact, max(loss_err), *max(tensors),
                                                     len(slices), *max(slices)))
  np.testing.assert_allclose(losses, ref.losses, rtol=1e-5)
  bad = [(err, what) for err, what in tensors + slices if not err <= TOL]
  assert not bad, sorted(bad, reverse=True)[:10]


def run_step(params, sub, idx, steps=1, **opts):
  """A fresh trainer stepped `steps` times over batch idx: per step (losses, flat_grads, flat_params)."""
  trainer = _capi.Trainer(params, **opts)
  try:
    trainer.set_data(sub)
    out = []
    for _ in range(steps):
      losses = trainer.step(idx)
      out.append((losses, trainer.flat_grads(), trainer.flat_params()))
    return out
  finally:
    trainer.close()


def bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('name,dropout', [('A', 0.0), ('B', 0.0), ('C', 0.0), ('D', 0.0), ('E', 0.0), ('E', 0.4)])
def test_gradients_match_float64_autograd(name, dropout):
  params, sub = make_case(name)
  hidden = SHAPES[name][1]
  ref = reference_of(name, dropout)
  assert ref.min_preact >= MIN_PREACT, ref.min_preact
  (losses, grads, _), = run_step(params, sub, batch_of(name), grad_max_norm=1e30, estimate_sigma2=True,
                                 dropout=dropout, dropout_key=KEY)
  compare('{} (dropout {})'.format(name, dropout), losses, grads, ref, hidden)


def test_zeros_move_the_mask_and_the_counts():
  """Case E's zeros reach what they are there for: in the reference's own terms, dimension 0 counts one
  row fewer than the rows present, every dimension misses the zero row, dimension 3 a whole column."""
  _, sub = make_case('E')
  idx = batch_of('E')
  truth = training.padded_batch(sub, idx)[1:].reshape(-1, SHAPES['E'][0])
  counts = (truth != 0).sum(axis=0)
  rows = sum(len(sub[i]) for i in idx)
  assert counts.tolist() == [rows - 2, rows - 1, rows - 1, rows - 1 - len(sub[2]), rows - 1]


@pytest.mark.parametrize('name', ['B', 'A'])
def test_clip_scales_the_core_gradients_only(name):
  """grad_max_norm at half the raw CoreRNN gradient norm scales exactly those gradients by
  max_norm / (norm + 1e-6); at twice the norm nothing changes.  A's norms have 770 partials each, so its
  coefficient depends on k_seg_norm_final's strided second pass."""
  params, sub = make_case(name)
  dim, hidden, depth = SHAPES[name][:3]
  idx = batch_of(name)
  n_rnn = train_ref.n_rnn(dim, hidden, depth)
  (raw_losses, raw, raw_p), = run_step(params, sub, idx, grad_max_norm=1e30)
  norm = np.linalg.norm(raw[:n_rnn].astype(np.float64))
  assert norm > 0
  (half_losses, half, _), = run_step(params, sub, idx, grad_max_norm=0.5 * norm)
  (twice_losses, twice, twice_p), = run_step(params, sub, idx, grad_max_norm=2.0 * norm)
  # float32(0.5 * norm) is what the kernel holds
  max_norm = float(np.float32(0.5 * norm))
  want = raw[:n_rnn].astype(np.float64) * train_ref.clip_coefficient(raw, n_rnn, max_norm)
  err = np.abs(half[:n_rnn] - want)
  worst = float(np.max(err / np.maximum(np.abs(want), 1e-300)))
  clipped = np.linalg.norm(half[:n_rnn].astype(np.float64))
  print('\nclip {}: raw norm {:.6g}, worst element {:.2e}, clipped norm / max_norm - 1 = {:.2e}'.format(
      name, norm, worst, clipped / max_norm - 1))
  assert np.all(err <= 1e-6 * np.abs(want)), worst
  assert clipped == pytest.approx(max_norm, rel=1e-5)
  assert np.array_equal(bits(half[n_rnn:]), bits(raw[n_rnn:]))  # rnn_init_hidden and sigma2: never clipped
  assert half_losses == raw_losses
  assert twice_losses == raw_losses
  assert np.array_equal(bits(twice), bits(raw))
  assert np.array_equal(bits(twice_p), bits(raw_p))


def test_adam_follows_a_float64_replay_of_its_own_gradients():
  """Five steps on one trainer.  Adam's moments and step sizes are replayed in float64 from the
  device's own (post-clip) gradients, which takes gradient error out of the comparison; each step's
  float64 update is added to the device's previous parameters, and
      |p_dev − p_ref| <= ulp32(p) + 1e-5 · |update|
  must hold after every step: one float32 rounding of the final sum, and about six float32 operations
  in the update (about 1e-6 relative together) with a factor of ten.  The step is taken from the
  device's previous parameters because the device rounds them once per step: against a float64
  trajectory from the start those roundings add up past one ulp without any defect."""
  params, sub = make_case('E')
  dim, hidden, depth = SHAPES['E'][:3]
  idx = batch_of('E')
  lr = 1e-2
  p0 = _capi.flatten_params(params)
  steps = run_step(params, sub, idx, steps=5, learning_rate=lr, grad_max_norm=0.5, dropout=0.4, dropout_key=KEY)
  sigma = train_ref.segments(dim, hidden, depth)[-1][1]
  replay = train_ref.adam_replay(p0, [g for _, g, _ in steps], lr, len(p0), sigma)
  prev_dev, prev_ref, worst = p0.astype(np.float64), p0.astype(np.float64), 0.0
  for (_, _, p_dev), p_ref in zip(steps, replay):
    update = p_ref - prev_ref
    assert np.all(p_ref[sigma] > 1e-6)  # no clamp here: the update is the whole step
    want = prev_dev + update
    bound = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 1e-5 * np.abs(update)
    err = np.abs(p_dev.astype(np.float64) - want)
    worst = max(worst, float(np.max(err / bound)))
    assert np.all(err <= bound), float(np.max(err / bound))
    assert np.count_nonzero(update) > 0.9 * len(update)
    prev_dev, prev_ref = p_dev.astype(np.float64), p_ref
  print('\nadam: worst |p_dev - p_ref| / bound over 5 steps {:.3f}'.format(worst))


# per-dimension data scale of the clamp test: small observations leave a small squared error, and with
# it a positive sigma2 gradient (the prior's a / sigma2 term wins); N(0,1) observations a negative one
CLAMP_SCALE = (0.1, 1.0, 0.1, 1.0, 1.0)


def test_sigma2_is_clamped_at_1e_6():
  """learning_rate 1.0 from sigma2 = 0.1: Adam's first step has size lr, so a dimension with a positive
  sigma2 gradient would land near -0.9 and must come out as float32(1e-6) exactly."""
  params, sub = make_case('E', None, CLAMP_SCALE)
  params = dict(params)
  params['sigma2'] = np.full(SHAPES['E'][0], 0.1, np.float32)
  idx = batch_of('E')
  padded = training.padded_batch(sub, idx)
  ref = train_ref.reference(params, padded, [len(sub[i]) + 1 for i in idx], {})
  sigma = ref.segments[-1][1]
  ref_grad = ref.flat[sigma]
  assert np.all(np.abs(ref_grad) > 1e-3), ref_grad  # no sign in doubt
  assert np.any(ref_grad > 0) and np.any(ref_grad < 0), ref_grad
  (_, grads, after), = run_step(params, sub, idx, learning_rate=1.0, grad_max_norm=1e30)
  assert np.array_equal(grads[sigma] > 0, ref_grad > 0)
  clamped = ref_grad > 0
  assert np.array_equal(bits(after[sigma][clamped]), bits(np.full(int(clamped.sum()), 1e-6, np.float32)))
  np.testing.assert_allclose(after[sigma][~clamped], 1.1, rtol=1e-6)


def test_estimate_sigma2_false_freezes_sigma2_only():
  params, sub = make_case('E')
  dim, hidden, depth = SHAPES['E'][:3]
  idx = batch_of('E')
  sigma = train_ref.segments(dim, hidden, depth)[-1][1]
  p0 = _capi.flatten_params(params)
  frozen = run_step(params, sub, idx, steps=3, learning_rate=1e-2, estimate_sigma2=False)
  free = run_step(params, sub, idx, steps=1, learning_rate=1e-2, estimate_sigma2=True)
  for _, grads, after in frozen:
    assert np.array_equal(bits(after[sigma]), bits(p0[sigma]))
    assert np.all(grads[sigma] != 0)  # the gradient is there; it is the update that is withheld
  assert not np.array_equal(bits(free[0][2][sigma]), bits(p0[sigma]))
  assert np.array_equal(bits(frozen[0][2][:sigma.start]), bits(free[0][2][:sigma.start]))
  assert not np.array_equal(bits(frozen[0][2][:sigma.start]), bits(p0[:sigma.start]))
  assert frozen[0][0] == free[0][0]


def _reuse_batches():
  """Batches over E's eight sub-sequences with (B, T) = (2, 4), (5, 12), (3, 3), (5, 12)."""
  return [[3, 4], [0, 1, 2, 3, 4], [5, 6, 7], [0, 1, 2, 3, 4]]


def test_one_trainer_across_batch_shapes():
  """The workspace is laid out anew for every batch inside a buffer that only grows.  With learning_rate 0
  (p + (-0)·x leaves the weights bit-exact) each step of one trainer must give the losses and gradients
  of a fresh trainer on that batch, bit for bit: nothing may depend on what an earlier layout left."""
  params, sub = make_case('E')
  batches = _reuse_batches()
  lengths = [[len(sub[i]) + 1 for i in idx] for idx in batches]
  assert [(len(l), l[0]) for l in lengths] == [(2, 4), (5, 12), (3, 3), (5, 12)]
  p0 = _capi.flatten_params(params)
  trainer = _capi.Trainer(params, learning_rate=0.0, grad_max_norm=1e30)
  try:
    trainer.set_data(sub)
    reused = []
    for idx in batches:
      losses = trainer.step(idx)
      reused.append((losses, trainer.flat_grads()))
      assert np.array_equal(bits(trainer.flat_params()), bits(p0))
  finally:
    trainer.close()
  for idx, (losses, grads) in zip(batches, reused):
    (fresh_losses, fresh_grads, _), = run_step(params, sub, idx, learning_rate=0.0, grad_max_norm=1e30)
    assert losses == fresh_losses, idx
    assert np.array_equal(bits(grads), bits(fresh_grads)), idx
    assert np.all(np.isfinite(grads)) and np.any(grads != 0)
  assert reused[1][0] == reused[3][0]
  assert np.array_equal(bits(reused[1][1]), bits(reused[3][1]))


def test_bad_batches_are_refused_and_leave_the_trainer_usable():
  params, sub = make_case('E')
  idx = batch_of('E')
  (want_losses, want_grads, want_params), = run_step(params, sub, idx, learning_rate=1e-2)
  trainer = _capi.Trainer(params, learning_rate=1e-2)
  try:
    trainer.set_data(sub)
    for bad in ([4, 3], [0, len(sub)], [-1], [0, 1, 2, 3, 4, 0]):
      with pytest.raises(_capi.HipLibraryError) as info:
        trainer.step(bad)
      assert info.value.status == _capi.UIS_ERR_INVALID_ARG, bad
    assert np.array_equal(bits(trainer.flat_params()), bits(_capi.flatten_params(params)))
    assert trainer.step(idx) == want_losses
    assert np.array_equal(bits(trainer.flat_grads()), bits(want_grads))
    assert np.array_equal(bits(trainer.flat_params()), bits(want_params))
  finally:
    trainer.close()
