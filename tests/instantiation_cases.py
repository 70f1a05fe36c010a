"""One decode per instantiation of the one-launch decode kernels: the case table of tests/test_gpu_instantiations.py,
built without a device (tests/test_instantiation_cases_host.py holds it to its own rules on the CPU).

uis_decoder.hip keeps seven tables of template instantiations (namespace kernels: rs, resident, big, big_ws, window,
deep, persist), keyed by (Hp, Dp, variant).  ROWS restates them by hand -- the host test asserts that the set equals
what the library enumerates (uis_decode_kernel_table), so a new instantiation without a case, or a case whose
instantiation is gone, fails there.  A row's key is what Decoder.last_instantiation() must report for its decodes:
(kernel family name, Hp, Dp, variant, persist).

Every row has one case per MODEL:
  exact    observation_dim == Dp, rnn_hidden_size == Hp
  padded   the smallest model uis_create pads to that entry (padded_dims restates its rule): hidden size 65 / 129 /
           385, observation dim 17 / 129 / 385 -- the most dead lanes and rows
  seg3     at Hp 512 also hidden size 257: segments of three k-blocks embedded in the 512 shape
The compile-time shape classes (variant != 0 outside deep) need the exact dims and their own beam / cap: the exact
model, and at 512 x 256 hidden size 257 with the exact observation dim, which the dispatch takes for unpadded too.
A UIS_FLAG_PERSISTENT session refuses padded frames: its padded models pad the hidden axis only.

Weights: synth.tracker_params where the hidden size holds the observation (H >= D; sigma2 0.05 instead of 0.005 beyond
256 dims, where the tracker otherwise spreads over tens of clusters), weights.init_params with a small sigma2 otherwise, the reference-trained trained_d512 checkpoint for the beam 20 / cap 11 class (its survivors stay
within that cap).  Utterances: ragged, one of a single frame, one of at least 2 * 16 + 1 decode steps where the row
leaves room, and a count that is no multiple of the device's XCD count `ncl` (so the XCDs hold different numbers).
How a row is reached (the thresholds are plan_decode's own):
  rs        at most 8 utterances per XCD, beam <= 16, beam * (cap + 1) <= 192
  resident  UIS_FLAG_OWNER_SELECT, at most 32 per XCD
  big_ws    20 * ncl + 1 utterances
  big       32 * ncl + 1 utterances, UIS_FLAG_OWNER_SELECT where Dp <= 256
  window    look_ahead 2, beam 4, three utterances (the beam 50 / cap 12 class: two of at most 12 frames)
  deep      rnn_depth 2; variant 1: look_ahead 2
  persist   a UIS_FLAG_PERSISTENT session fed in uneven pushes (test_iteration 1: online decoding)
The many-utterance rows use lengths 1 .. 7 and test_iteration 1, the others test_iteration 2.
"""

import functools
import os

import numpy as np

import golden_util
from uisrnn_amd import _capi
from uisrnn_amd import synth
from uisrnn_amd import weights

# variants (uis_decoder.hip: CLS_*, RS_*)
CLS_NONE, CLS_C1, CLS_C4, CLS_C2 = 0, 1, 2, 3
RS_BASE, RS_C1 = 1, 2

RS, RESIDENT, BIG, BIG_WS, WINDOW, DEEP = ('k_decode_rs', 'k_decode_resident', 'k_decode_big', 'k_decode_big<WS>',
                                           'k_decode_big<WIN>', 'k_decode_deep')

_D256 = [(512, 256), (512, 128), (256, 256), (256, 128), (128, 256), (128, 128)]
_D512 = [(512, 512), (256, 512), (128, 512)]

# (family, Hp, Dp, variant, persist): every entry of the seven tables
ROWS = (
    [(RS, hp, dp, RS_BASE, 0) for hp, dp in _D256] + [(RS, 512, 256, RS_C1, 0)] +
    [(RESIDENT, hp, dp, CLS_NONE, 0) for hp, dp in _D256 + _D512] +
    [(RESIDENT, 512, 256, CLS_C1, 0), (RESIDENT, 512, 512, CLS_C4, 0)] +
    [(BIG, hp, dp, CLS_NONE, 0) for hp, dp in _D256 + _D512] +
    [(BIG_WS, hp, dp, CLS_NONE, 0) for hp, dp in _D256] + [(BIG_WS, 512, 256, CLS_C1, 0)] +
    [(WINDOW, hp, dp, CLS_NONE, 0) for hp, dp in _D256 + _D512] + [(WINDOW, 512, 256, CLS_C2, 0)] +
    [(DEEP, hp, dp, 0, 0) for hp, dp in [(512, 256), (512, 128), (512, 512), (256, 256), (256, 128), (128, 128), (128, 256)]] +
    [(DEEP, hp, dp, 1, 0) for hp, dp in [(512, 256), (256, 256), (256, 128), (128, 128)]] +
    [(RESIDENT, hp, dp, CLS_NONE, 1) for hp, dp in [(512, 256), (512, 512), (256, 256)]])

_SHORT = {RS: 'rs', RESIDENT: 'resident', BIG: 'big', BIG_WS: 'big_ws', WINDOW: 'window', DEEP: 'deep'}


def row_id(row):
  family, hp, dp, variant, persist = row
  return '{}-H{}-D{}-v{}'.format('persist' if persist else _SHORT[family], hp, dp, variant)


# the select limits, restated from the kernels' headers (uis_kernels.hip: select_fast_ok; uis_select_rs.hip: UIS_RS_MAXB,
# UIS_RS_MAXC, UIS_RS_MAXS, rs_select_ok)
def select_fast_ok(beam, cap):
  return beam <= 64 and beam * (cap + 1) <= 256 and beam * cap + beam <= 1024


def rs_select_ok(beam, cap, max_steps):
  return beam <= 16 and beam * (cap + 1) <= 192 and beam * cap + beam <= 256 and max_steps < 65535


def padded_dims(dim, hidden):
  """uis_create's padding rule: (Dp, Hp), or None where the model keeps its sizes rounded up to 16 (no cluster kernel).
  q = ceil(blocks of 16 / 8) is the canonical K-segment length; padding keeps it."""
  d16, h16 = -(-dim // 16) * 16, -(-hidden // 16) * 16
  qh, qd = -(-(h16 // 16) // 8), -(-(d16 // 16) // 8)
  hp = 128 if (qh == 1 and hidden > 64) else 256 if qh == 2 else 512 if qh in (3, 4) else 0
  dp = 128 if d16 <= 128 else 256 if qd == 2 else 512 if qd == 4 else 0
  return (dp, hp) if hp and dp else None


_BARELY = {128: 65, 256: 129, 512: 385}     # hidden sizes
_BARELY_D = {128: 17, 256: 129, 512: 385}   # observation dims

_FEW = (17, 1, 9, 5, 12, 3, 20, 7, 14, 2, 11)        # test_iteration 2: 34 decode steps in the longest
_SESSION = (33, 1, 12, 7, 20, 3, 16, 9, 26, 5, 14)   # test_iteration 1


class Case:
  """One decode: a model, its utterances as a function of the XCD count, and the options that reach the row."""

  def __init__(self, row, model, dim, hidden, **kw):
    self.row, self.model, self.dim, self.hidden = row, model, dim, hidden
    self.depth = kw.get('depth', 1)
    self.beam = kw['beam']
    self.cap = kw['cap']
    self.look_ahead = kw.get('look_ahead', 1)
    self.test_iteration = kw.get('test_iteration', 2)
    self.flags = kw.get('flags', 0)
    self.count = kw['count']            # ncl -> number of utterances
    self.lengths = kw['lengths']        # the cycle the lengths are taken from
    self.checkpoint = kw.get('checkpoint')
    self.nodedup = kw.get('nodedup', False)   # also decoded under UIS_FLAG_NO_DEDUP
    self.session = bool(row[4])
    self.seed = kw.get('seed', 0)
    self.sigma2 = kw.get('sigma2', 0.02)   # of an init_params model
    self.name = '{}/{}'.format(row_id(row), model)

  def n_utt(self, ncl):
    return self.count(ncl)

  def lens(self, ncl):
    n = self.n_utt(ncl)
    return [self.lengths[u % len(self.lengths)] for u in range(n)]

  def params(self):
    return _params(self.dim, self.hidden, self.depth, self.checkpoint, self.seed, self.sigma2)

  def utterances(self, ncl):
    return _utterances(self.dim, tuple(self.lens(ncl)), self.seed, bool(self.checkpoint))

  def pushes(self, ncl):
    """Sessions: per push, the number of new frames of each utterance (uneven, at most 16 a push)."""
    left = self.lens(ncl)
    sizes, out, k = (1, 7, 3, 16, 5, 2, 11), [], 0
    while any(left):
      take = [min(sizes[(k + u) % len(sizes)], n) for u, n in enumerate(left)]
      left = [n - t for n, t in zip(left, take)]
      out.append(take)
      k += 1
    return out


@functools.lru_cache(maxsize=None)
def _params(dim, hidden, depth, checkpoint, seed, sigma2):
  if checkpoint:
    return weights.load_checkpoint(os.path.join(golden_util.GOLDEN_DIR, checkpoint))
  if hidden >= dim:
    # (the 512-dim tracker spreads over tens of clusters at its default sigma2: a wider one keeps it inside the caps)
    return synth.tracker_params(dim, hidden, depth, seed=3 + seed, sigma2=0.05 if dim > 256 else 0.005)
  params = weights.init_params(dim, hidden, depth, sigma2=sigma2, transition_bias=0.05, crp_alpha=1.0,
                               seed=dim + hidden + seed)
  params['rnn_init_hidden'] = (0.2 * np.random.default_rng(7).standard_normal((depth, hidden))).astype(np.float32)
  return params


@functools.lru_cache(maxsize=None)
def _utterances(dim, lens, seed, trained):
  """Unit-norm speaker centroids (what the tracker weights and the trained checkpoint were made for; a fresh
  init_params model opens a handful of clusters on them too): for the checkpoint the segments it was trained on, else
  four speakers and a change every five frames or so."""
  if trained:
    return synth.make_utterances(8300 + seed, len(lens), list(lens), dim)[0]
  return [synth.make_utterance(8100 + dim + seed + u, n, dim, num_speakers=4, mean_segment=5.0)[0]
          for u, n in enumerate(lens)]


def _many(u):
  return 1 + (3 * u) % 7


_MANY = tuple(_many(u) for u in range(7))   # lengths 1 .. 7

# Seeds other than 0, picked on the CPU until the case meets the host test's conditions (three clusters in some
# hypothesis, the survivors inside the cap).
_SEEDS = {'window-H128-D256-v0/exact': 2, 'window-H512-D512-v0/seg3': 6, 'window-H256-D512-v0/padded': 2,
          'window-H256-D512-v0/exact': 10}
# ... and a smaller sigma2 where no seed opens a third cluster
_SIGMA2 = {'window-H256-D512-v0/exact': 0.005}


def _models(row):
  """(model name, observation dim, hidden size) of a row's cases."""
  family, hp, dp, variant, persist = row
  if variant == RS_C1 if family == RS else (variant != 0 and family != DEEP):
    # (hidden size 257 with the exact observation dim looks unpadded to the dispatch too: every unit mask open)
    return [('exact', dp, hp)] + ([('seg3', dp, 257)] if (hp, dp) == (512, 256) else [])
  d_pad = dp if persist else _BARELY_D[dp]
  out = [('exact', dp, hp), ('padded', d_pad, _BARELY[hp])]
  if hp == 512:
    out.append(('seg3', d_pad, 257))
  return out


def cases_of(row):
  family, hp, dp, variant, persist = row
  owner = _capi.UIS_FLAG_OWNER_SELECT
  out = []
  for model, dim, hidden in _models(row):
    # (observation dim 385 .. 512: the models spread over more clusters)
    kw = dict(beam=8, cap=16 if dp == 512 else 12, lengths=_FEW, count=lambda ncl: 2 * ncl + 3)
    if persist:
      kw.update(flags=_capi.UIS_FLAG_PERSISTENT, test_iteration=1, lengths=_SESSION, count=lambda ncl: ncl + 3)
    elif family == RS:
      if variant == RS_C1:
        kw.update(beam=10, cap=16, nodedup=True)
    elif family == RESIDENT:
      kw.update(flags=owner)
      if variant == CLS_C1:
        kw.update(beam=10, cap=16, nodedup=True)
      elif variant == CLS_C4:
        kw.update(beam=20, cap=11, nodedup=True, checkpoint='trained_d512.uisrnn')
    elif family == BIG_WS:
      kw.update(beam=6, cap=10, test_iteration=1, lengths=_MANY, count=lambda ncl: 20 * ncl + 1)
      if variant == CLS_C1:
        kw.update(beam=10, cap=16, nodedup=True)
    elif family == BIG:
      kw.update(beam=6, cap=10, test_iteration=1, lengths=_MANY, count=lambda ncl: 32 * ncl + 1,
                flags=owner if dp <= 256 else 0, nodedup=(hp, dp) == (512, 256) and model == 'exact')
    elif family == WINDOW:
      kw.update(beam=4, cap=12 if dp == 512 else 8, look_ahead=2, lengths=(17, 1, 9), count=lambda ncl: 3)
      if variant == CLS_C2:
        kw.update(beam=50, cap=12, lengths=(12, 1), count=lambda ncl: 2, nodedup=True)
    elif family == DEEP:
      kw.update(depth=2, beam=6, cap=20 if dp == 512 else 12, count=lambda ncl: ncl + 3,
                nodedup=(hp, dp, variant) == (512, 256, 0) and model == 'exact')
      if variant == 1:
        kw.update(beam=4, cap=8, look_ahead=2, lengths=(17, 1, 9), count=lambda ncl: 3)
    kw['seed'] = _SEEDS.get('{}/{}'.format(row_id(row), model), 0)
    kw['sigma2'] = _SIGMA2.get('{}/{}'.format(row_id(row), model), 0.02)
    out.append(Case(row, model, dim, hidden, **kw))
  return out


CASES = {row: cases_of(row) for row in ROWS}
