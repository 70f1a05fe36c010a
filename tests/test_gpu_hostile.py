"""Every decode kernel family on saturating, subnormal, overflowing and tie-ridden numerics (tests/hostile.py),
bit for bit against the oracle: labels, scores, the whole final beam, max_clusters_seen -- and the kernel the
library says it ran, so nothing falls back silently.  Each case first proves on the CPU that its regime was
reached (hostile.reached); only then does it look at the device's output.

What the device is held to here and nowhere else: include/uis_numerics.h's contract is IEEE add / mul / div /
fma / rint WITH SUBNORMALS KEPT.  A flush-to-zero compile flag, a reciprocal in place of a division or a moved
branch threshold changes bits only on inputs like these.

The table (x = decoded and compared; saturated = both gains where "40/200", the x 200 one where "200"):

  family                                   edges  saturated  subnormal  overflow  sigma_small  sigma_large
  k_decode_rs fixed    D256 H512 b10 c16     x     40/200       x          x          x            x
  k_decode_rs generic  D128 H256 b5  c20     x      200         x
  k_decode_rs padded   D72  H300 b10 c16     x      200         x
  k_decode_resident    the three above,      x     40/200       x          x          x            x     (D256)
                       UIS_FLAG_OWNER_SELECT x      200         x                                        (D128, D72)
  k_decode_resident    D512 H512 b20         x      200         x
  k_decode_big<WS>     D256 H512, 161 utt    x      200         x
  k_decode_big<WIN>    D256 H512 look 2      x      200         x
  k_decode_deep        D48  H256 depth 2     x      200         x
  k_decode_small       D16 H8, D33 H17,      x     40/200       x          x          x            x     (D16 H8)
                       depth 1 / 2, look 2   x      200         x                                        (the others)
  launch per step      D256 H512             x     40/200       x          x          x            x
    + SMALL_TILES, > 2048 rows, beam 40      x      200         x
  generic window       D256 H512 b12 look 3  x      200         x

Conditions: NaNs are compared as "NaN in the same places" (x86 and gfx950 differ in the default NaN's sign),
everything else by bit pattern, so a -0.0 must stay -0.0 (in frames and scores; a gate pre-activation is never -0.0: every
dense chain ends by adding its +0.0 segments).  The k_decode_small shapes have fewer hidden units than the edge list has
entries: D16 H8 runs edges at 29 offsets, D33 H17 depth 2 at nine, which between them hand every gate every edge.  k_decode_big<WS> needs a whole MI355X (256 compute
units) to be selected and is skipped elsewhere, as the dispatch crossover test is.  Utterances are 8 .. 15 frames
(8 .. 10 at beam 20) so that no hypothesis can reach the cluster caps the shape classes fix.
"""

import functools

import numpy as np
import pytest

import forced_ref
import hostile
from oracle import oracle
from uisrnn_amd import _capi

pytestmark = pytest.mark.gpu

CORE = hostile.REGIMES
MUST = ('edges', 'saturated200', 'subnormal')
OWNER, RES, STEP, SMALL_TILES = (_capi.UIS_FLAG_OWNER_SELECT, _capi.UIS_FLAG_RESIDENT, _capi.UIS_FLAG_STEPWISE,
                                 _capi.UIS_FLAG_SMALL_TILES)
RS_GENERIC, RS_FIXED = 1, 2


def _lengths(n_utt, lo=8, hi=15):
  return tuple(lo + (5 * u) % (hi - lo + 1) for u in range(n_utt))


# family -> shape, beam, look_ahead, max_clusters (None: what the oracle's survivors needed, plus look_ahead),
# flags, lengths, the kernel the library must name (a prefix), k_decode_rs's kind, regimes, edges offsets
FAMILIES = {
    'rs_fixed': dict(shape=(256, 512, 1), beam=10, cap=16, lengths=_lengths(16), want='k_decode_rs', kind=RS_FIXED, regimes=CORE),
    'rs_generic': dict(shape=(128, 256, 1), beam=5, cap=20, lengths=_lengths(12, 8, 19), want='k_decode_rs', kind=RS_GENERIC),
    'rs_padded': dict(shape=(72, 300, 1), beam=10, cap=16, lengths=_lengths(10), want='k_decode_rs', kind=RS_GENERIC),
    'resident_fixed': dict(shape=(256, 512, 1), beam=10, cap=16, lengths=_lengths(16), flags=OWNER, want='k_decode_resident', regimes=CORE),
    'resident_generic': dict(shape=(128, 256, 1), beam=5, cap=20, lengths=_lengths(12, 8, 19), flags=OWNER, want='k_decode_resident'),
    'resident_padded': dict(shape=(72, 300, 1), beam=10, cap=16, lengths=_lengths(10), flags=OWNER, want='k_decode_resident'),
    'resident_d512': dict(shape=(512, 512, 1), beam=20, lengths=_lengths(8, 8, 10), want='k_decode_resident'),
    'big_ws': dict(shape=(256, 512, 1), beam=10, cap=16, lengths=(8,) * 161, want='k_decode_big<WS>', whole_device=True),
    'big_win': dict(shape=(256, 512, 1), beam=10, look=2, lengths=_lengths(6), want='k_decode_big<WIN>'),
    'deep': dict(shape=(48, 256, 2), beam=6, lengths=_lengths(9), flags=RES, want='k_decode_deep'),
    'small_h8': dict(shape=(16, 8, 1), beam=4, lengths=_lengths(9), flags=RES, want='k_decode_small', regimes=CORE, offsets=tuple(range(0, 116, 4))),
    'small_h17_depth2': dict(shape=(33, 17, 2), beam=6, lengths=_lengths(9), flags=RES, want='k_decode_small', offsets=tuple(range(0, 116, 13))),
    'small_h8_depth2': dict(shape=(16, 8, 2), beam=4, lengths=_lengths(5), flags=RES, want='k_decode_small'),
    'small_h17_look2': dict(shape=(33, 17, 1), beam=4, look=2, lengths=_lengths(6), flags=RES, want='k_decode_small'),
    'stepwise': dict(shape=(256, 512, 1), beam=10, cap=16, lengths=_lengths(16), flags=STEP, want='stepwise', regimes=CORE),
    'stepwise_small_tiles': dict(shape=(256, 512, 1), beam=10, cap=16, lengths=_lengths(16), flags=STEP | SMALL_TILES, want='stepwise'),
    'stepwise_wide': dict(shape=(256, 512, 1), beam=10, cap=16, lengths=_lengths(224, 8, 10), flags=STEP, want='stepwise:k_wt'),
    'stepwise_beam40': dict(shape=(256, 512, 1), beam=40, lengths=_lengths(4), flags=STEP, want='stepwise'),
    'window_generic': dict(shape=(256, 512, 1), beam=12, look=3, lengths=_lengths(4, 8, 10), flags=STEP, want='stepwise'),
}

_CASES = [(fam, regime, offset) for fam, spec in FAMILIES.items() for regime in spec.get('regimes', MUST)
          for offset in (spec.get('offsets', (0,)) if regime == 'edges' else (0,))]


def test_the_table_meets_its_conditions():
  """Every family sees edges, saturated and subnormal; every regime sees k_decode_rs, k_decode_resident,
  k_decode_small and the launch-per-step path; the small models' edges offsets are those the host test checks."""
  for fam, spec in FAMILIES.items():
    assert set(MUST) <= set(spec.get('regimes', MUST)), fam
  for regime in hostile.REGIMES:
    seen = {FAMILIES[f]['want'] for f, r, _ in _CASES if r == regime}
    assert {'k_decode_rs', 'k_decode_resident', 'k_decode_small', 'stepwise'} <= seen, regime
  small = {FAMILIES[f]['shape'] + (o,) for f, r, o in _CASES
           if r == 'edges' and FAMILIES[f]['want'] == 'k_decode_small'}
  assert set(hostile.SMALL_EDGE_CASES) <= small


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
  """Bit for bit, except that a NaN only has to be a NaN."""
  got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
  assert got.shape == want.shape, what
  nan = np.isnan(want)
  assert np.array_equal(np.isnan(got), nan), what + ': NaN in different places'
  assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), what


@functools.lru_cache(maxsize=None)
def _case(regime, shape, lengths, offset):
  return hostile.build(regime, shape[0], shape[1], shape[2], lengths=lengths, offset=offset)


@functools.lru_cache(maxsize=None)
def _reference(regime, shape, lengths, offset, beam, look):
  """The oracle's decode of a case (test_iteration 1) and the regime's check, once for all families that share it."""
  oracle.lib()
  case = _case(regime, shape, lengths, offset)
  ref = oracle.decode(case.params, case.seqs, beam, look, 1, n_threads=8)
  ref1 = ref if look == 1 else oracle.decode(case.params, case.seqs, beam, 1, 1, n_threads=8)
  hostile.reached(case, oracle, ref1, beam)
  return ref


def _whole_device():
  import torch  # (only for the device's compute-unit count)
  return torch.cuda.get_device_properties(0).multi_processor_count == 256


@pytest.mark.parametrize('family,regime,offset', _CASES, ids=['{}-{}-{}'.format(*c) for c in _CASES])
def test_decode_bit_exact(family, regime, offset, oracle_lib):
  spec = FAMILIES[family]
  if spec.get('whole_device') and not _whole_device():
    pytest.skip('not a whole MI355X')
  look = spec.get('look', 1)
  case = _case(regime, spec['shape'], spec['lengths'], offset)
  ref = _reference(regime, spec['shape'], spec['lengths'], offset, spec['beam'], look)   # (asserts the regime)
  seen = max(int(ref['max_clusters'].max()), 1)
  cap = spec.get('cap') or max(seen + look, 4)
  assert seen < cap, 'the case itself would hit the cluster cap'
  frames, offsets = oracle_lib.pack(case.seqs)
  dec = _capi.Decoder(case.params)
  out = dec.decode(frames, offsets, spec['beam'], look, 1, max_clusters=cap, flags=spec.get('flags', 0),
                   want_beam_scores=True)
  dec.close()
  assert out['status'] == 0 and not out['overflow'].any()
  assert out['stats']['decode_kernel'].startswith(spec['want']), out['stats']['decode_kernel']
  if 'kind' in spec:
    assert (out['stats']['decode_kernel_code'] >> 16) & 0xff == spec['kind'], hex(out['stats']['decode_kernel_code'])
  for u in range(len(case.seqs)):
    assert np.array_equal(out['labels'][offsets[u]:offsets[u + 1]], ref['labels'][u]), 'labels differ, utterance %d' % u
  _same(out['scores'], ref['scores'], 'scores')
  _same(out['beam_scores'], ref['beam_scores'], 'final beam')
  assert out['stats']['max_clusters_seen'] == seen


_STEP_SHAPES = [(fam, regime) for fam in ('rs_fixed', 'rs_generic', 'rs_padded', 'resident_d512', 'deep', 'small_h8',
                                          'small_h17_depth2')
                for regime in ('edges', 'saturated40', 'saturated200')]


@pytest.mark.parametrize('family,regime', _STEP_SHAPES)
def test_rnn_step_on_the_edges_and_saturated_models(family, regime, oracle_lib):
  """Decoder.rnn_step: the oracle's bits, and within the a priori bound of decode_ref64.step."""
  spec = FAMILIES[family]
  case = _case(regime, spec['shape'], spec['lengths'], 0)
  _reference(regime, spec['shape'], spec['lengths'], 0, spec['beam'], 1)
  rows = hostile.step_rows(case, oracle_lib)
  dec = _capi.Decoder(case.params)
  got = [dec.rnn_step(x, h) for x, h in rows]
  m0, h1 = dec.constants()
  dec.close()
  for (x, h), (mean, hout) in zip(rows, got):
    mean_o, hout_o = oracle_lib.rnn_step(case.params, x, h)
    _same(mean, mean_o, 'mean')
    _same(hout, hout_o, 'hidden state')
  m0_o, h1_o = oracle_lib.constants(case.params)
  _same(m0, m0_o, 'm0')
  _same(h1, h1_o, 'h1')
  it = iter(got)
  hostile.check_step(case, rows, lambda x, h: next(it))


@pytest.mark.parametrize('regime', hostile.REGIMES)
@pytest.mark.parametrize('family', ['rs_fixed', 'small_h17_depth2'])
def test_score_labels(family, regime, oracle_lib):
  """score_labels with per-frame losses on the oracle's labels and on an alternating labeling: forced_ref.score's
  bits (a +inf frame is +inf on both sides), within the a priori bound of decode_ref64.forced_nll, and on the
  decode's own labels the decode's score, bit for bit."""
  spec = FAMILIES[family]
  case = _case(regime, spec['shape'], spec['lengths'], 0)
  ref = _reference(regime, spec['shape'], spec['lengths'], 0, spec['beam'], 1)
  frames, offsets = oracle_lib.pack(case.seqs)
  dec = _capi.Decoder(case.params)
  got = {name: dec.score_labels(frames, offsets, np.concatenate(labels), want_frame_losses=True)
         for name, labels in hostile.labelings(case, ref).items()}
  cap = spec.get('cap') or max(int(ref['max_clusters'].max()) + 1, 4)
  out = dec.decode(frames, offsets, spec['beam'], 1, 1, max_clusters=cap, flags=spec.get('flags', 0))
  dec.close()
  live = np.array([(l >= 0).all() for l in ref['labels']])
  assert live.any()
  for name, labels in hostile.labelings(case, ref).items():
    scores, losses = got[name]
    ref_scores, ref_losses = forced_ref.score(case.params, case.seqs, labels)
    _same(scores, ref_scores, name + ': totals')
    _same(losses, np.concatenate(ref_losses), name + ': per-frame losses')
    per_utt = [losses[offsets[u]:offsets[u + 1]] for u in range(len(case.seqs))]
    _, compared, _ = hostile.check_forced(case, labels, scores, per_utt, utterances=(0, 1, 2, 3))
    assert compared >= 4
  _same(got['oracle'][0][live], out['scores'][live], 'the decode\'s own score')
  if regime == 'overflow':
    assert np.isposinf(got['alternating'][1]).any() and np.isfinite(got['alternating'][1]).any()


@pytest.mark.parametrize('persistent', [False, True], ids=['plain', 'persistent'])
@pytest.mark.parametrize('regime', hostile.REGIMES)
def test_streaming_session_equals_the_offline_decode(regime, persistent, oracle_lib):
  """One session per regime on the k_decode_rs shape, pushes of 1 and of 7 frames in turn: the final labels,
  scores and beams are the offline decode's, which are the oracle's."""
  spec = FAMILIES['rs_fixed']
  case = _case(regime, spec['shape'], spec['lengths'], 0)
  ref = _reference(regime, spec['shape'], spec['lengths'], 0, spec['beam'], 1)
  frames, offsets = oracle_lib.pack(case.seqs)
  dec = _capi.Decoder(case.params)
  off = dec.decode(frames, offsets, spec['beam'], 1, 1, max_clusters=spec['cap'], want_beam_scores=True)
  dec.stream_begin(len(case.seqs), spec['beam'], max(spec['lengths']), max_clusters=spec['cap'],
                   flags=_capi.UIS_FLAG_PERSISTENT if persistent else 0)
  try:
    pos = [0] * len(case.seqs)
    push = 0
    while any(p < len(s) for p, s in zip(pos, case.seqs)):
      take = 1 if push % 2 == 0 else 7
      chunks = []
      for u, s in enumerate(case.seqs):
        n = min(take, len(s) - pos[u])
        chunks.append(np.asarray(s[pos[u]:pos[u] + n], dtype=np.float32) if n else None)
        pos[u] += n
      dec.stream_push(chunks)
      push += 1
    labels, scores, overflow, status = dec.stream_labels()
    beam = np.empty((len(case.seqs), spec['beam']), dtype=np.float32)
    dec._check(dec._lib.uis_last_decode_info(dec._handle, None, beam.ctypes.data_as(_capi._fp)), 'info')  # pylint: disable=protected-access
  finally:
    dec.stream_end()
  dec.close()
  assert status == 0 and not overflow.any()
  for u in range(len(case.seqs)):
    assert np.array_equal(labels[u], off['labels'][offsets[u]:offsets[u + 1]]), u
    assert np.array_equal(labels[u], ref['labels'][u]), u
  _same(scores, off['scores'], 'scores against the offline decode')
  _same(scores, ref['scores'], 'scores against the oracle')
  _same(beam, off['beam_scores'], 'final beam')
