"""GPU parity: the HIP decoder against the CPU oracle, bit for bit.

Every call goes through the C ABI (uisrnn_amd._capi -> libuisrnn_hip.so).
Labels are compared exactly; scores and the whole final beam are compared as
float32 BIT PATTERNS -- both sides follow include/uis_numerics.h, so any
difference is a bug, not round-off.  (Agreement of the oracle with the
reference itself is tests/test_oracle_golden.py, run on CPU; relative
tolerance 1e-4 there, as BASELINE.json's north_star states.)
"""

import numpy as np
import pytest

import golden_util
from uisrnn_amd import _capi
from uisrnn_amd import synth
from uisrnn_amd import weights

pytestmark = pytest.mark.gpu


_PATH_FLAGS = (_capi.UIS_FLAG_STEPWISE | _capi.UIS_FLAG_RESIDENT | _capi.UIS_FLAG_GRAPH |
               _capi.UIS_FLAG_SMALL_TILES)


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _compare(params, seqs, beam_size, look_ahead, test_iteration, oracle_lib,
             flags=0, max_clusters=0, decoder=None, n_streams=0):
  ref = oracle_lib.decode(params, seqs, beam_size, look_ahead, test_iteration,
                          n_threads=8)
  dec = decoder or _capi.Decoder(params)
  frames, offsets = oracle_lib.pack(seqs)
  cap = max(int(ref['max_clusters'].max()) if len(seqs) else 1, 1)
  # Where the one-launch decode (k_decode_resident) applies it is the default; a call that
  # does not pick a path itself is checked on BOTH paths.
  variants = [flags]
  if not flags & _PATH_FLAGS and look_ahead == 1 and n_streams in (0, 1):
    variants.append(flags | _capi.UIS_FLAG_STEPWISE)
    # ... and, where the replicated select (k_decode_rs) is the default, with the select of an
    # utterance on one workgroup (k_decode_resident) as well
    variants.append(flags | _capi.UIS_FLAG_OWNER_SELECT)
  elif not flags & _PATH_FLAGS and n_streams in (0, 1):
    # look_ahead >= 2: one launch (k_decode_big<WIN>) where it applies, and a launch per sub-step
    variants.append(flags | _capi.UIS_FLAG_STEPWISE)
  for fl in variants:
    # intermediate look-ahead levels hold hypotheses with up to look_ahead - 1 more clusters
    # than any survivor
    out = dec.decode(frames, offsets, beam_size, look_ahead, test_iteration,
                     max_clusters=max_clusters or max(cap + look_ahead - 1, 4),
                     flags=fl,
                     want_beam_scores=True, n_streams=n_streams)
    assert out['status'] == 0
    assert not out['overflow'].any()
    for u in range(len(seqs)):
      got = out['labels'][offsets[u]:offsets[u + 1]]
      assert np.array_equal(got, ref['labels'][u]), 'labels differ, utterance %d' % u
    assert np.array_equal(_bits(out['scores']), _bits(ref['scores']))
    assert np.array_equal(_bits(out['beam_scores']), _bits(ref['beam_scores']))
    assert out['stats']['max_clusters_seen'] == cap
  return out, ref


def test_same_numerics_version(oracle_lib):
  """Both binaries were built from the same include/uis_numerics.h."""
  assert (_capi.load_library().uis_numerics_version() ==
          oracle_lib.numerics_version())


def test_rnn_step_bit_exact(oracle_lib):
  """CoreRNN.forward (uisrnn.py:45-52): kernels vs oracle, and vs the reference's outputs."""
  for name in ('tiny_d16', 'toy_d2_depth2', 'd32_lookahead3', 'd20_h24_depth3',
               'tracker_d256', 'tracker_d64_h300'):   # (the last: hidden size 300, embedded in the 512-wide kernels: round 6)
    case = golden_util.load_case(name)
    dec = _capi.Decoder(case['params'])
    unit = case['unit']
    for x, h, mean_ref, h_ref in zip(unit['unit_x'], unit['unit_h'],
                                     unit['unit_mean'], unit['unit_hout']):
      mean, hout = dec.rnn_step(x, h)
      mean_o, hout_o = oracle_lib.rnn_step(case['params'], x, h)
      assert np.array_equal(_bits(mean), _bits(mean_o))
      assert np.array_equal(_bits(hout), _bits(hout_o))
      np.testing.assert_allclose(mean, mean_ref, rtol=1e-4, atol=1e-6)
      np.testing.assert_allclose(hout, h_ref, rtol=1e-4, atol=1e-6)
    m0, h1 = dec.constants()
    m0_o, h1_o = oracle_lib.constants(case['params'])
    assert np.array_equal(_bits(m0), _bits(m0_o))
    assert np.array_equal(_bits(h1), _bits(h1_o))


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2', 'd32_lookahead3',
                                  'd20_h24_depth3', 'tracker_d256_long', 'tracker_d64_h300'])
def test_golden_cases_bit_exact(name, oracle_lib):
  case = golden_util.load_case(name)
  dec = _capi.Decoder(case['params'])
  for run in case['runs']:
    out, _ = _compare(case['params'], case['seqs'], run['beam_size'],
                      run['look_ahead'], run['test_iteration'], oracle_lib,
                      decoder=dec)
    # and against the reference's own outputs stored in the fixture
    offsets = np.cumsum([0] + [len(s) for s in case['seqs']])
    for u in range(len(case['seqs'])):
      assert np.array_equal(out['labels'][offsets[u]:offsets[u + 1]],
                            run['labels'][u])
    np.testing.assert_allclose(out['scores'], run['best'], rtol=1e-4)


def test_tracker_golden_look_ahead(oracle_lib):
  """D=256/H=512 fixture (labels and scores recorded from the reference), L = 1 and 2."""
  case = golden_util.load_case('tracker_d256')
  dec = _capi.Decoder(case['params'])
  for run in case['runs']:
    out, _ = _compare(case['params'], case['seqs'], run['beam_size'],
                      run['look_ahead'], run['test_iteration'], oracle_lib,
                      decoder=dec)
    offsets = np.cumsum([0] + [len(s) for s in case['seqs']])
    for u in range(len(case['seqs'])):
      assert np.array_equal(out['labels'][offsets[u]:offsets[u + 1]],
                            run['labels'][u])
    np.testing.assert_allclose(out['scores'], run['best'], rtol=1e-4)


def test_look_ahead_wide_beam(oracle_lib):
  """BASELINE config #3 shape at a size the oracle finishes: beam 50, look_ahead 2."""
  params = synth.tracker_params(256, 512, 1, seed=0)
  seqs, _ = synth.make_utterances(7000, 3, [30, 17, 24], 256)
  out, _ = _compare(params, seqs, 50, 2, 2, oracle_lib, max_clusters=12)
  assert out['stats']['rnn_rows'] < out['stats']['rnn_rows_nodedup']
  _compare(params, seqs[:2], 20, 3, 1, oracle_lib, max_clusters=8)


@pytest.mark.parametrize('dim,hidden', [(256, 512), (128, 256), (512, 512)])
def test_look_ahead_in_one_launch(dim, hidden, oracle_lib):
  """look_ahead >= 2 with every sub-step of every window in ONE launch (k_decode_big<WIN>: the
  window kernel's sub-step as the select stage), ragged utterances, against the oracle and the
  launch-per-sub-step path, bit for bit; also with more utterances than workgroups."""
  params = synth.tracker_params(dim, hidden, 1, seed=5)
  lengths = [23, 9, 30, 1, 14, 2, 27, 18, 5, 21, 16]
  seqs, _ = synth.make_utterances(5000 + dim, len(lengths), lengths, dim)
  dec = _capi.Decoder(params)
  # (max_clusters from the oracle's run: the 512-dim tracker spreads over tens of clusters)
  out, ref = _compare(params, seqs, 10, 2, 1, oracle_lib, decoder=dec)
  assert out['stats']['decode_kernel'].startswith('stepwise')  # (_compare's last variant)
  frames, offsets = oracle_lib.pack(seqs)
  one = dec.decode(frames, offsets, 10, 2, 1, max_clusters=int(ref['max_clusters'].max()) + 1,
                   want_beam_scores=True)
  assert one['stats']['decode_kernel'] == 'k_decode_big<WIN>'
  _compare(params, seqs[:5], 6, 3, 2, oracle_lib, decoder=dec)
  _compare(params, seqs[:3], 25, 2, 1, oracle_lib, decoder=dec)
  if dim == 256:
    many = [seqs[i % len(seqs)][:8] for i in range(300)]
    f2, o2 = oracle_lib.pack(many)
    big = dec.decode(f2, o2, 4, 2, 1, max_clusters=6, want_beam_scores=True)
    assert big['stats']['decode_kernel'] == 'k_decode_big<WIN>'  # (a workgroup runs its utterances' windows in turn)
    step = dec.decode(f2, o2, 4, 2, 1, max_clusters=6, want_beam_scores=True, flags=_capi.UIS_FLAG_STEPWISE)
    assert np.array_equal(big['labels'], step['labels'])
    assert np.array_equal(_bits(big['beam_scores']), _bits(step['beam_scores']))
    ref = oracle_lib.decode(params, many[:len(seqs)], 4, 2, 1, n_threads=8)
    for u in range(len(seqs)):
      assert np.array_equal(big['labels'][o2[u]:o2[u + 1]], ref['labels'][u])


@pytest.mark.parametrize('dim,hidden', [(250, 200), (100, 400), (40, 500), (512, 130), (64, 256),
                                        (256, 100), (100, 128), (400, 70),
                                        (256, 300), (120, 320), (256, 384), (64, 257), (500, 370)])
def test_in_between_sizes_take_the_one_launch_kernels(dim, hidden, oracle_lib):
  """rnn_depth 1, hidden size 65 .. 512, observation dim up to 256 / 385 .. 512: the
  library pads the model up to the cluster kernels' shapes (128 / 256 / 512 x 128 / 256 / 512) -- the
  canonical K-segment length is the same there, so the oracle (which pads to 16) is matched bit for
  bit -- and the decode is one launch, look_ahead 1 and 2.  Round 6: hidden sizes 257 .. 384 (segments of three
  k-blocks) too, embedded in the 512 shape with a zero block behind every segment (uis_decoder.hip: HidMap;
  tests/test_padding_exact.py proves the claim on the oracle) -- they ran a launch per step before."""
  from uisrnn_amd import weights
  params = weights.init_params(dim, hidden, 1, sigma2=0.1, transition_bias=0.2, crp_alpha=1.0, seed=dim + hidden)
  params['rnn_init_hidden'] = (0.2 * np.random.default_rng(7).standard_normal((1, hidden))).astype(np.float32)
  rng = np.random.default_rng(dim * 1000 + hidden)
  cents = rng.standard_normal((3, dim))
  seqs = []
  for n in (23, 7, 31, 1, 16, 12, 20, 9, 28):
    ids = np.repeat(rng.integers(0, 3, size=n // 4 + 1), 4)[:n]
    seqs.append((cents[ids] * 0.4 + 0.1 * rng.standard_normal((n, dim))).astype(np.float64))
  dec = _capi.Decoder(params)
  _, ref = _compare(params, seqs, 8, 1, 2, oracle_lib, decoder=dec)
  frames, offsets = oracle_lib.pack(seqs)
  cap = int(ref['max_clusters'].max()) + 1
  out = dec.decode(frames, offsets, 8, 1, 2, max_clusters=cap)
  assert out['status'] == 0
  if 8 * (cap + 1) <= 256:  # (the select's LDS budget; an untrained model can spread over many clusters)
    assert out['stats']['decode_kernel'].startswith('k_decode_r')
  _, ref = _compare(params, seqs[:4], 5, 2, 1, oracle_lib, decoder=dec)
  f4, o4 = oracle_lib.pack(seqs[:4])
  out = dec.decode(f4, o4, 5, 2, 1, max_clusters=int(ref['max_clusters'].max()) + 2)
  assert out['status'] == 0 and out['stats']['decode_kernel'] == 'k_decode_big<WIN>'
  # CoreRNN.forward on the padded model
  x = rng.standard_normal(dim).astype(np.float32)
  h0 = rng.standard_normal((1, hidden)).astype(np.float32)
  mean, hout = dec.rnn_step(x, h0)
  mean_o, hout_o = oracle_lib.rnn_step(params, x, h0)
  assert np.array_equal(_bits(mean), _bits(mean_o)) and np.array_equal(_bits(hout), _bits(hout_o))


@pytest.mark.parametrize('hidden', [320, 384])
def test_embedded_hidden_sizes_on_the_shape_class_kernels(hidden, oracle_lib):
  """rnn_hidden_size 257 .. 384 embedded in the 512 shape (round 6) with observation_dim 256, beam 10 and the default
  cluster cap: the model then looks unpadded to the dispatch (every unit mask open) and takes the compile-time shape
  classes of BASELINE configs[1] / [3] -- k_decode_rs's class for 40 utterances, k_decode_big<WS>'s for 300 -- and the
  launch-per-step path under UIS_FLAG_STEPWISE: all three equal the oracle, bit for bit."""
  from uisrnn_amd import weights
  params = weights.init_params(256, hidden, 1, sigma2=0.02, transition_bias=0.05, crp_alpha=1.0, seed=hidden)
  params['rnn_init_hidden'] = (0.2 * np.random.default_rng(3).standard_normal((1, hidden))).astype(np.float32)
  dec = _capi.Decoder(params)
  for n_utt, want in ((40, 'k_decode_rs'), (300, 'k_decode_big<WS>')):
    lens = [6 + (5 * u) % 19 for u in range(n_utt)]
    seqs, _ = synth.make_utterances(19_000 + hidden + n_utt, n_utt, lens, 256)
    frames, offsets = oracle_lib.pack(seqs)
    ref = oracle_lib.decode(params, seqs, 10, 1, 2, n_threads=8)
    cap = max(int(ref['max_clusters'].max()), 16)
    for flags in (0, _capi.UIS_FLAG_STEPWISE):
      out = dec.decode(frames, offsets, 10, 1, 2, max_clusters=cap, want_beam_scores=True, flags=flags)
      assert out['status'] == 0
      if cap == 16 and not flags:
        assert out['stats']['decode_kernel'] == want, out['stats']['decode_kernel']
      assert np.array_equal(out['labels'], np.concatenate(ref['labels'])), (n_utt, flags)
      assert np.array_equal(_bits(out['beam_scores']), _bits(ref['beam_scores'])), (n_utt, flags)


def test_tracker_d256_bit_exact(oracle_lib):
  params = synth.tracker_params(256, 512, 1, seed=0)
  seqs, _ = synth.make_utterances(2000, 12, [50, 80, 31, 64, 17, 100, 1, 2, 77,
                                             45, 90, 33], 256)
  out, _ = _compare(params, seqs, 10, 1, 2, oracle_lib)
  assert out['stats']['rnn_rows'] <= out['stats']['rnn_rows_nodedup']


def test_dedup_flag_is_bit_identical(oracle_lib):
  params = synth.tracker_params(256, 512, 1, seed=3)
  seqs, _ = synth.make_utterances(3000, 6, [40, 55, 23, 64, 9, 70], 256)
  a, _ = _compare(params, seqs, 10, 1, 2, oracle_lib)
  b, _ = _compare(params, seqs, 10, 1, 2, oracle_lib,
                  flags=_capi.UIS_FLAG_NO_DEDUP)
  assert b['stats']['rnn_rows'] == b['stats']['rnn_rows_nodedup']
  assert a['stats']['rnn_rows'] < b['stats']['rnn_rows']


def test_streams_and_graph_are_bit_identical(oracle_lib):
  """Utterance groups on several streams and hipGraph replay change scheduling only."""
  params = synth.tracker_params(256, 512, 1, seed=1)
  lengths = [70, 33, 64, 12, 90, 41, 5, 77, 64, 20, 51]
  seqs, _ = synth.make_utterances(4000, len(lengths), lengths, 256)
  dec = _capi.Decoder(params)
  for n_streams, flags in ((1, 0), (3, 0), (1, _capi.UIS_FLAG_GRAPH),
                           (4, _capi.UIS_FLAG_GRAPH), (8, 0)):
    out, _ = _compare(params, seqs, 10, 1, 2, oracle_lib, decoder=dec,
                      flags=flags, n_streams=n_streams)
    assert out['stats']['n_streams'] == n_streams


def test_wide_tiles_bit_exact(oracle_lib):
  """row capacity > 2048 switches the launch-per-step dense kernels to a wave per row tile: with
  hidden size 256 / 512 the kernels that keep their weight slice in LDS (k_wt_*), else the big-tile
  ones that stream it (k_big_*); UIS_FLAG_SMALL_TILES keeps the split-K kernels in their 2x2 tile
  shape.  Also two-layer models (k_dense_upper_in feeds the GRU kernel of either kind)."""
  params = synth.tracker_params(256, 512, 1, seed=2)
  n_utt = 224
  lengths = [10 + (7 * u) % 23 for u in range(n_utt)]
  seqs, _ = synth.make_utterances(6000, n_utt, lengths, 256)
  _compare(params, seqs, 10, 1, 2, oracle_lib)
  _compare(params, seqs, 10, 1, 2, oracle_lib, flags=_capi.UIS_FLAG_STEPWISE | _capi.UIS_FLAG_SMALL_TILES)
  deep = synth.tracker_params(128, 128, 2, seed=12)       # depth 2: never the one-launch decode
  seqs2, _ = synth.make_utterances(6100, n_utt, [8 + (5 * u) % 11 for u in range(n_utt)], 128)
  _compare(deep, seqs2, 10, 1, 1, oracle_lib)
  _compare(deep, seqs2, 10, 1, 1, oracle_lib, flags=_capi.UIS_FLAG_SMALL_TILES)
  deep2 = synth.tracker_params(128, 256, 2, seed=13)      # depth 2, hidden 256: k_wt_gru for both layers
  _compare(deep2, seqs2, 10, 1, 1, oracle_lib)


def test_generic_select_flag_is_bit_identical(oracle_lib):
  """k_select_fast (default where it applies) and the general k_select agree with the oracle."""
  params = synth.tracker_params(256, 512, 1, seed=4)
  seqs, _ = synth.make_utterances(8000, 9, [60, 33, 80, 12, 45, 1, 64, 27, 50], 256)
  _compare(params, seqs, 10, 1, 2, oracle_lib)
  _compare(params, seqs, 10, 1, 2, oracle_lib, flags=_capi.UIS_FLAG_GENERIC_SELECT)
  _compare(params, seqs, 32, 1, 1, oracle_lib, max_clusters=7)     # 32 * 8 = 256 candidates: fast path limit
  _compare(params, seqs, 70, 1, 1, oracle_lib, max_clusters=8)     # beyond it: general kernel


def test_resident_decode_is_bit_identical(oracle_lib):
  """UIS_FLAG_RESIDENT: the whole decode in one launch (k_decode_resident) vs the oracle."""
  params = synth.tracker_params(256, 512, 1, seed=6)
  lengths = [64, 30, 77, 12, 50, 41, 1, 90, 23, 64, 35, 18]      # ragged, not a multiple of 8
  seqs, _ = synth.make_utterances(8800, len(lengths), lengths, 256)
  dec = _capi.Decoder(params)
  for _ in range(3):  # in-launch hand-offs are timing dependent: repeat
    _compare(params, seqs, 10, 1, 2, oracle_lib, decoder=dec, flags=_capi.UIS_FLAG_RESIDENT)
  _compare(params, seqs[:3], 10, 1, 2, oracle_lib, decoder=dec, flags=_capi.UIS_FLAG_RESIDENT)  # idle XCDs
  _compare(params, seqs[:1], 4, 1, 3, oracle_lib, decoder=dec, flags=_capi.UIS_FLAG_RESIDENT)
  many, _ = synth.make_utterances(8900, 300, 12, 256)   # several utterances per workgroup, > 3 row tiles per XCD
  _compare(params, many, 10, 1, 1, oracle_lib, flags=_capi.UIS_FLAG_RESIDENT | _capi.UIS_FLAG_NO_DEDUP)
  _compare(params, many, 20, 1, 1, oracle_lib, flags=_capi.UIS_FLAG_RESIDENT)
  wide = synth.tracker_params(512, 512, 1, seed=7)      # observation_dim 512: one linear_mean2 tile per rank
  seqs5, _ = synth.make_utterances(8950, 20, 25, 512)
  _compare(wide, seqs5, 8, 1, 2, oracle_lib, flags=_capi.UIS_FLAG_RESIDENT)   # up to 26 clusters per hypothesis
  small = synth.tracker_params(256, 256, 1, seed=8)     # hidden 256: two ranks share a GRU / linear_mean1 tile
  many256, _ = synth.make_utterances(8960, 300, 11, 256)
  _compare(small, many256, 10, 1, 1, oracle_lib, flags=_capi.UIS_FLAG_RESIDENT)
  _compare(small, seqs, 10, 1, 2, oracle_lib, flags=_capi.UIS_FLAG_RESIDENT)
  # hidden size 24, depth 3: a small model -- its one-launch decode is k_decode_small (round 4)
  case = golden_util.load_case('d20_h24_depth3')
  d2 = _capi.Decoder(case['params'])
  out = d2.decode(*oracle_lib.pack(case['seqs']), 6, 1, 2, flags=_capi.UIS_FLAG_RESIDENT)
  assert out['status'] == 0 and out['stats']['decode_kernel'] == 'k_decode_small'
  with pytest.raises(_capi.HipLibraryError):  # hidden size 600: beyond the cluster kernels' shapes (257 .. 384 are embedded since round 6): must be refused
    from uisrnn_amd import weights
    p3 = weights.init_params(40, 600, 1, sigma2=0.1, transition_bias=0.2, seed=3)
    s3 = [np.random.default_rng(3).standard_normal((9, 40))]
    _capi.Decoder(p3).decode(*oracle_lib.pack(s3), 6, 1, 2, flags=_capi.UIS_FLAG_RESIDENT)
  # look_ahead 2 on the small model: one launch too (k_decode_small with a window sub-step as its select)
  out = d2.decode(*oracle_lib.pack(case['seqs']), 6, 2, 2, flags=_capi.UIS_FLAG_RESIDENT)
  assert out['status'] == 0 and out['stats']['decode_kernel'] == 'k_decode_small'
  with pytest.raises(_capi.HipLibraryError):  # look_ahead 2, hidden size 600: no one-launch kernel
    _capi.Decoder(p3).decode(*oracle_lib.pack(s3), 6, 2, 2, flags=_capi.UIS_FLAG_RESIDENT)


@pytest.mark.parametrize('dim,hidden', [(256, 512), (256, 256), (512, 512), (128, 256)])
def test_one_launch_decode_with_more_utterances_than_workgroups(dim, hidden, oracle_lib):
  """More than 256 utterances: k_decode_big (a wave per row tile, weights in LDS) against the
  split-K passes of k_decode_resident (UIS_FLAG_SMALL_TILES) and the launch-per-step path, ragged
  lengths, bit for bit; a sample against the oracle."""
  import os
  from uisrnn_amd import weights
  trained = os.path.join(golden_util.GOLDEN_DIR, 'trained_d{}.uisrnn'.format(dim))
  # (the closed-form tracker weights open clusters without end at observation_dim 512)
  params = weights.load_checkpoint(trained) if hidden == 512 and os.path.exists(trained) else synth.tracker_params(dim, hidden, 1, seed=41)
  lens = [5 + (7 * u) % 40 for u in range(300)]
  seqs, _ = synth.make_utterances(13_000, len(lens), lens, dim)
  dec = _capi.Decoder(params)
  frames, offsets = oracle_lib.pack(seqs)
  big = dec.decode(frames, offsets, 10, 1, 2, want_beam_scores=True, flags=_capi.UIS_FLAG_RESIDENT)
  assert big['status'] == 0 and big['stats']['kernel_launches']['select'] == 0
  assert big['stats']['decode_kernel'] == ('k_decode_big<WS>' if dim <= 256 else 'k_decode_big'), big['stats']['decode_kernel']
  # (UIS_FLAG_COHORTS: accepted and ignored -- the decode is the default one, bit for bit)
  for flags in (_capi.UIS_FLAG_RESIDENT | _capi.UIS_FLAG_SMALL_TILES, _capi.UIS_FLAG_STEPWISE,
                _capi.UIS_FLAG_RESIDENT | _capi.UIS_FLAG_COHORTS, _capi.UIS_FLAG_RESIDENT | _capi.UIS_FLAG_OWNER_SELECT):
    other = dec.decode(frames, offsets, 10, 1, 2, want_beam_scores=True, flags=flags)
    assert np.array_equal(big['labels'], other['labels']), flags
    assert np.array_equal(_bits(big['beam_scores']), _bits(other['beam_scores'])), flags
    assert np.array_equal(_bits(big['scores']), _bits(other['scores'])), flags
    assert other['stats']['rnn_rows'] == big['stats']['rnn_rows'], flags
    if flags & _capi.UIS_FLAG_COHORTS:
      assert other['stats']['decode_kernel'] == ('k_decode_big<WS>' if dim <= 256 else 'k_decode_big'), flags
  sample = [0, 37, 151, 299]
  ref = oracle_lib.decode(params, [seqs[u] for u in sample], 10, 1, 2, n_threads=4)
  for k, u in enumerate(sample):
    assert np.array_equal(big['labels'][offsets[u]:offsets[u + 1]], ref['labels'][k]), u
    assert np.array_equal(_bits(big['beam_scores'][u]), _bits(ref['beam_scores'][k])), u


def test_dispatch_crossovers_name_their_kernels(oracle_lib):
  """Which one-launch kernel decodes how many utterances (uis_stats.decode_kernel; the library's rule, retuned in
  round 5 from profiles/r05_usweep_dispatch.json): at most 8 per XCD the replicated select, up to 20 per XCD the
  owner-select kernel, from 21 on the wave-per-row-tile kernel with concurrent single-wave selects; where those
  do not apply (observation dim 512) the owner-select kernel up to 32 per XCD.  Every batch against the
  launch-per-step path bit for bit."""
  import os
  from uisrnn_amd import weights
  ncl = 8  # (a whole MI355X: 256 compute units in clusters of 32)
  cases = [('trained_d256.uisrnn', 256, 10, 16, [(8 * ncl, 'k_decode_rs'), (8 * ncl + 1, 'k_decode_resident'), (20 * ncl, 'k_decode_resident'),
                                                 (20 * ncl + 1, 'k_decode_big<WS>'), (32 * ncl + 1, 'k_decode_big<WS>')]),
           ('trained_d512.uisrnn', 512, 20, 11, [(8 * ncl + 1, 'k_decode_resident'), (32 * ncl, 'k_decode_resident'), (32 * ncl + 1, 'k_decode_big')])]
  for ckpt, dim, beam, cap, points in cases:
    params = weights.load_checkpoint(os.path.join(golden_util.GOLDEN_DIR, ckpt))
    dec = _capi.Decoder(params)
    import torch  # (only for the device's compute-unit count)
    if torch.cuda.get_device_properties(0).multi_processor_count != 32 * ncl:
      pytest.skip('not a whole MI355X')
    for n_utt, want in points:
      lens = [3 + (5 * u) % 9 for u in range(n_utt)]
      seqs, _ = synth.make_utterances(31_000 + n_utt, n_utt, lens, dim)
      frames, offsets = oracle_lib.pack(seqs)
      one = dec.decode(frames, offsets, beam, 1, 1, max_clusters=cap, want_beam_scores=True)
      assert one['status'] == 0 and one['stats']['decode_kernel'] == want, (n_utt, one['stats']['decode_kernel'], want)
      step = dec.decode(frames, offsets, beam, 1, 1, max_clusters=cap, want_beam_scores=True, flags=_capi.UIS_FLAG_STEPWISE)
      assert np.array_equal(one['labels'], step['labels']) and np.array_equal(_bits(one['beam_scores']), _bits(step['beam_scores'])), n_utt


def test_resident_decode_falls_back_when_its_placement_check_fails(oracle_lib):
  """The one-launch decode verifies its own assumptions (XCD placement, barrier progress); a
  failed check must cost a re-run on the launch-per-step path, not an error or a wrong answer."""
  params = synth.tracker_params(256, 512, 1, seed=9)
  seqs, _ = synth.make_utterances(9100, 10, [40, 12, 33, 64, 5, 21, 50, 17, 30, 8], 256)
  dec = _capi.Decoder(params)
  _compare(params, seqs, 10, 1, 2, oracle_lib, decoder=dec,
           flags=_capi.UIS_FLAG_NO_DEDUP | _capi.UIS_FLAG_TEST_MISPLACED)
  st = dec.decode(*oracle_lib.pack(seqs), 10, 1, 2, flags=_capi.UIS_FLAG_PROFILE)['stats']
  assert st['kernel_launches']['select'] > 0          # this handle now stays on the per-step path
  with pytest.raises(_capi.HipLibraryError):          # demanded explicitly: the failure is reported
    _capi.Decoder(params).decode(*oracle_lib.pack(seqs), 10, 1, 2,
                                 flags=_capi.UIS_FLAG_RESIDENT | _capi.UIS_FLAG_TEST_MISPLACED)
  # (round 5) ... also when the decode was going to be several launches with the later frames travelling behind the
  # first: the re-run brings the whole list to the device again
  same, _ = synth.make_utterances(9200, 12, 150, 256)
  ref = oracle_lib.decode(params, same, 10, 1, 1, n_threads=6)
  for entry in ('f32', 'f64'):
    dec2 = _capi.Decoder(params)
    cap = max(int(ref['max_clusters'].max()), 4)
    out = (dec2.decode(*oracle_lib.pack(same), 10, 1, 1, max_clusters=cap, flags=_capi.UIS_FLAG_TEST_MISPLACED, want_beam_scores=True) if entry == 'f32'
           else dec2.decode_f64(same, 10, 1, 1, max_clusters=cap, flags=_capi.UIS_FLAG_TEST_MISPLACED, want_beam_scores=True))
    assert out['status'] == 0 and out['stats']['decode_kernel'].startswith('stepwise') and out['stats']['decode_launches'] == 0
    assert np.array_equal(out['labels'], np.concatenate(ref['labels'])) and np.array_equal(_bits(out['beam_scores']), _bits(ref['beam_scores']))


def test_one_launch_decode_gives_up_on_a_silent_workgroup(oracle_lib):
  """The hand-offs of k_decode_rs are polls of words other workgroups write; UIS_FLAG_TEST_STALL
  makes one workgroup stop writing its word after three steps.  The waves that wait for it must give
  up (about a second), every workgroup must leave the launch, and the call must come back with the
  launch-per-step path's answer -- or, when the one-launch decode was demanded, with an error."""
  import time
  params = synth.tracker_params(256, 512, 1, seed=9)
  seqs, _ = synth.make_utterances(9150, 10, [40, 12, 33, 64, 5, 21, 50, 17, 30, 8], 256)
  ref = oracle_lib.decode(params, seqs, 10, 1, 2, n_threads=8)
  frames, offsets = oracle_lib.pack(seqs)
  dec = _capi.Decoder(params)
  t0 = time.time()
  out = dec.decode(frames, offsets, 10, 1, 2, flags=_capi.UIS_FLAG_TEST_STALL, want_beam_scores=True)
  assert time.time() - t0 < 20.0
  assert out['status'] == 0
  for u in range(len(seqs)):
    assert np.array_equal(out['labels'][offsets[u]:offsets[u + 1]], ref['labels'][u])
  assert np.array_equal(_bits(out['beam_scores']), _bits(ref['beam_scores']))
  st = dec.decode(frames, offsets, 10, 1, 2, flags=_capi.UIS_FLAG_PROFILE)['stats']
  assert st['kernel_launches']['select'] > 0          # this handle now stays on the per-step path
  with pytest.raises(_capi.HipLibraryError, match='timed out'):
    _capi.Decoder(params).decode(frames, offsets, 10, 1, 2, flags=_capi.UIS_FLAG_RESIDENT | _capi.UIS_FLAG_TEST_STALL)


@pytest.mark.parametrize('dim,beam,n_utt', [(256, 10, 64), (256, 10, 100), (512, 20, 64)],
                         ids=['k_decode_rs', 'k_decode_resident_256', 'k_decode_resident_512'])
def test_phase_words_published_at_either_scope_give_the_same_bits(dim, beam, n_utt, oracle_lib):
  """Round 6: UIS_FLAG_AGENT_FLAGS stores the per-producer phase words of the dense-stage hand-offs with AGENT scope -- the
  HIP memory model's by-the-book form -- instead of the workgroup-scope store that stays in the XCD's L2 (the default: the
  conforming store costs a third of the step, profiles/r06_agent_flags_ab.txt).  A run-time choice in ONE binary (it was
  a compile-time variant): same kernel, same bits, against each other and the oracle."""
  import os
  from uisrnn_amd import weights as wts
  params = wts.load_checkpoint(os.path.join(golden_util.GOLDEN_DIR, 'trained_d{}.uisrnn'.format(dim)))  # (BASELINE configs[1] / [4])
  lens = [30 + (13 * u) % 25 for u in range(n_utt)]
  seqs, _ = synth.make_utterances(17_000 + n_utt, n_utt, lens, dim)
  frames, offsets = oracle_lib.pack(seqs)
  dec = _capi.Decoder(params)
  cap = 11 if beam == 20 else 16
  base = dec.decode(frames, offsets, beam, 1, 2, want_beam_scores=True, max_clusters=cap, flags=_capi.UIS_FLAG_RESIDENT)
  agent = dec.decode(frames, offsets, beam, 1, 2, want_beam_scores=True, max_clusters=cap, flags=_capi.UIS_FLAG_RESIDENT | _capi.UIS_FLAG_AGENT_FLAGS)
  assert base['status'] == 0 and agent['status'] == 0
  assert agent['stats']['decode_kernel'] == base['stats']['decode_kernel']
  assert base['stats']['decode_kernel'] in ('k_decode_rs', 'k_decode_resident'), base['stats']['decode_kernel']
  assert np.array_equal(base['labels'], agent['labels'])
  assert np.array_equal(_bits(base['beam_scores']), _bits(agent['beam_scores']))
  sample = [0, n_utt // 2, n_utt - 1]
  ref = oracle_lib.decode(params, [seqs[u] for u in sample], beam, 1, 2, n_threads=3)
  for k, u in enumerate(sample):
    assert np.array_equal(agent['labels'][offsets[u]:offsets[u + 1]], ref['labels'][k]), u
    assert np.array_equal(_bits(agent['beam_scores'][u]), _bits(ref['beam_scores'][k])), u


def test_quirk7_zero_first_difference_on_the_device(oracle_lib):
  """weighted_mse_loss returns inf when the FIRST squared difference is exactly 0
  (uisrnn/loss_func.py:36,41: nnz counts the first column only).  Engineered on the decode
  path: a frame whose component 0 equals m0[0] makes the fresh-cluster candidate's MSE inf
  (k_mse0); a frame whose component 0 equals a live cluster's mean[0] does the same for that
  cluster (the select's MSE).  Both decode paths must agree with the oracle bit for bit."""
  params = synth.tracker_params(256, 512, 1, seed=0)
  dec = _capi.Decoder(params)
  m0, _ = dec.constants()
  seqs, _ = synth.make_utterances(9300, 2, [14, 9], 256)
  seqs[0][0, 0] = np.float64(m0[0])    # the very first frame: its only candidate is non-finite
  seqs[1][4, 0] = np.float64(m0[0])    # mid-utterance: the fresh cluster drops out of that step
  out, ref = _compare(params, seqs, 10, 1, 1, oracle_lib, decoder=dec)
  assert (ref['labels'][0] == -1).all()          # the beam emptied at step 0, like the reference's
  assert (ref['labels'][1] >= 0).all()
  assert np.isinf(oracle_lib.weighted_mse(params, m0, seqs[0][0].astype(np.float32)))
  # a live cluster's mean: after one frame the cluster's mean is the network's output for it
  x0 = seqs[1][0].astype(np.float32)
  _, h1 = dec.constants()
  mean1, _ = dec.rnn_step(x0, h1)
  probe = [np.array(seqs[1][:3])]
  probe[0][1, 0] = np.float64(mean1[0])          # frame 1 meets cluster 0's mean[0] exactly
  _, ref2 = _compare(params, probe, 10, 1, 1, oracle_lib, decoder=dec)
  assert ref2['labels'][0].tolist()[1] != 0      # staying in cluster 0 was non-finite: a new one opens


def test_exact_ties_on_the_device(oracle_lib):
  """Exactly equal candidate scores (tests/golden/probes.json 'exact_ties', recorded from the
  reference): the select kernels' lowest-flat-index rule gives the reference's labels, on the
  one-launch path (no: these tiny shapes run launch-per-step), the fast and the general select."""
  import json
  import os
  with open(os.path.join(golden_util.GOLDEN_DIR, 'probes.json')) as f:
    probes = json.load(f)
  for probe in probes['exact_ties']:
    dim, hidden, beam, n_frames, seed, look = probe['spec']
    params, seq = golden_util.tie_probe_case(dim, hidden, beam, n_frames, seed)
    dec = _capi.Decoder(params)
    frames, offsets = oracle_lib.pack([seq])
    ref = oracle_lib.decode(params, [seq], beam, look, 1)
    for flags in (0, _capi.UIS_FLAG_GENERIC_SELECT):
      out = dec.decode(frames, offsets, beam, look, 1, want_beam_scores=True, flags=flags)
      assert out['status'] == 0
      assert out['labels'].tolist() == probe['labels'], (probe['spec'], flags)
      assert np.array_equal(_bits(out['beam_scores']), _bits(ref['beam_scores']))
  for probe in probes['exact_ties_unstable']:   # (the reference's unstable argsort chose differently: equal scores)
    dim, hidden, beam, n_frames, seed, look = probe['spec']
    params, seq = golden_util.tie_probe_case(dim, hidden, beam, n_frames, seed)
    params['crp_alpha'] = probe['crp_alpha']
    dec = _capi.Decoder(params)
    frames, offsets = oracle_lib.pack([seq])
    ref = oracle_lib.decode(params, [seq], beam, look, 1)
    out = dec.decode(frames, offsets, beam, look, 1, max_clusters=32, want_beam_scores=True)
    assert out['status'] == 0
    assert out['labels'].tolist() == probe['decoder_labels'], probe['spec']
    assert np.array_equal(_bits(out['beam_scores']), _bits(ref['beam_scores']))


def test_level_capacity_is_reported_not_retried(oracle_lib):
  """look_ahead >= 2: when a window has more live prefixes than an intermediate level holds the
  call fails with UIS_ERR_UNSUPPORTED and says so (doubling max_clusters could not help)."""
  params, rng = _many_cluster_case()
  seqs = [rng.standard_normal((14, 64))]
  dec = _capi.Decoder(params)
  frames, offsets = oracle_lib.pack(seqs)
  with pytest.raises(_capi.HipLibraryError, match='look-ahead window'):
    dec.decode(frames, offsets, 200, 4, 1, max_clusters=30)   # 200 * 31 * 32 * 33 prefixes > 32768


def test_decode_while_another_stream_keeps_cus_busy(oracle_lib):
  """The one-launch decode spins on in-launch barriers.  It is launched cooperatively, so the
  runtime either makes all its workgroups co-resident or refuses; with other kernels occupying
  the device (here: torch matmuls on another stream, before, during and after) the results must
  stay identical -- whether the launch waits, or the barrier guard triggers the fallback."""
  import torch
  params = synth.tracker_params(256, 512, 1, seed=11)
  seqs, _ = synth.make_utterances(9400, 16, 40, 256)
  ref = oracle_lib.decode(params, seqs, 10, 1, 2, n_threads=8)
  dec = _capi.Decoder(params)
  frames, offsets = oracle_lib.pack(seqs)
  side = torch.cuda.Stream()
  a = torch.randn(4096, 4096, device='cuda')
  for _ in range(4):
    with torch.cuda.stream(side):
      for _ in range(30):
        a = torch.tanh(a @ a) * 0.01
    out = dec.decode(frames, offsets, 10, 1, 2)
    assert out['status'] == 0
    for u in range(len(seqs)):
      assert np.array_equal(out['labels'][offsets[u]:offsets[u + 1]], ref['labels'][u])
    assert np.array_equal(_bits(out['scores']), _bits(ref['scores']))
  torch.cuda.synchronize()


def test_host_buffer_decode_from_pinned_memory(oracle_lib):
  """uis_decode from pinned host buffers (uis_host_alloc): chunked H2D overlapped with the input
  projection gives the same labels as the pageable path."""
  import ctypes
  params = synth.tracker_params(256, 512, 1, seed=0)
  seqs, _ = synth.make_utterances(9450, 40, 300, 256)   # 12000 frames: several copy chunks
  frames, offsets = oracle_lib.pack(seqs)
  dec = _capi.Decoder(params)
  want = dec.decode(frames, offsets, 10, 1, 2)
  lib = _capi.load_library()
  bufs = []
  for nbytes in (frames.nbytes, 4 * len(frames), 4 * len(seqs)):
    p = ctypes.c_void_p()
    assert lib.uis_host_alloc(nbytes, ctypes.byref(p)) == 0
    bufs.append(p)
  try:
    ctypes.memmove(bufs[0], frames.ctypes.data, frames.nbytes)
    rc = dec.decode_host(bufs[0].value, offsets, 10, 1, 2, bufs[1].value, bufs[2].value)
    assert rc['status'] == 0
    got = np.ctypeslib.as_array(ctypes.cast(bufs[1], ctypes.POINTER(ctypes.c_int32)), (len(frames),))
    assert np.array_equal(got, want['labels'])
    sc = np.ctypeslib.as_array(ctypes.cast(bufs[2], ctypes.POINTER(ctypes.c_float)), (len(seqs),))
    assert np.array_equal(_bits(sc), _bits(want['scores']))
  finally:
    for p in bufs:
      lib.uis_host_free(p)


def _many_cluster_case():
  """Untrained weights + a large crp_alpha open clusters freely (31 in 40 frames)."""
  from uisrnn_amd import weights  # pylint: disable=import-outside-toplevel
  params = weights.init_params(64, 48, 1, sigma2=0.5, transition_bias=0.5,
                               crp_alpha=50.0, seed=5)
  rng = np.random.default_rng(6)
  return params, rng


def test_random_weights_many_clusters(oracle_lib):
  """Cluster-cap stress: far more clusters than the default table size."""
  params, rng = _many_cluster_case()
  seqs = [rng.standard_normal((n, 64)) for n in (40, 45, 12)]
  _, ref = _compare(params, seqs, 8, 1, 2, oracle_lib)
  assert ref['max_clusters'].max() > 16


def test_free_switching_model_on_the_one_launch_decode(oracle_lib):
  """The single-wave select's prune keeps what scores at or below the worst 'stay' candidate; a
  model that switches speakers as readily as it stays (transition_bias 0.5, a flat observation
  noise) leaves long short lists -- beyond 16, 32 and 64 survivors: every counting pass of the
  short list and the fall-back rounds -- with beam 16 and 8 utterances per cluster."""
  from uisrnn_amd import weights  # pylint: disable=import-outside-toplevel
  for seed, sigma2, alpha in ((21, 4.0, 1.0), (22, 0.5, 8.0), (23, 50.0, 0.3)):
    params = weights.init_params(256, 512, 1, sigma2=sigma2, transition_bias=0.5, crp_alpha=alpha, seed=seed)
    rng = np.random.default_rng(seed + 100)
    seqs = [0.3 * rng.standard_normal((n, 256)) for n in (60, 48, 33, 60, 7, 52, 41, 60, 29)]
    _compare(params, seqs, 16, 1, 2, oracle_lib)


def test_cluster_cap_is_reported(oracle_lib):
  params, rng = _many_cluster_case()
  seqs = [rng.standard_normal((40, 64)), rng.standard_normal((3, 64))]
  ref = oracle_lib.decode(params, seqs, 8, 1, 2)
  assert ref['max_clusters'][0] > 8 and ref['max_clusters'][1] <= 8
  dec = _capi.Decoder(params)
  frames, offsets = oracle_lib.pack(seqs)
  out = dec.decode(frames, offsets, 8, 1, 2, max_clusters=8)
  assert out['status'] == _capi.UIS_ERR_CLUSTER_CAP
  assert out['overflow'].tolist() == [1, 0]
  # the utterance that fit is still decoded correctly
  assert np.array_equal(out['labels'][offsets[1]:offsets[2]], ref['labels'][1])


def test_cluster_cap_on_the_one_launch_decode(oracle_lib):
  """Hidden size 512 (the one-launch decode): a hypothesis that outgrows max_clusters is flagged
  per utterance exactly like on the launch-per-step path, and the doubled retry of the Python
  host gives the oracle's labels."""
  import uisrnn_amd
  from uisrnn_amd import weights  # pylint: disable=import-outside-toplevel
  params = weights.init_params(256, 512, 1, sigma2=0.5, transition_bias=0.5, crp_alpha=50.0, seed=15)
  rng = np.random.default_rng(16)
  seqs = [rng.standard_normal((30, 256)), rng.standard_normal((2, 256)), rng.standard_normal((25, 256))]
  ref = oracle_lib.decode(params, seqs, 8, 1, 2, n_threads=3)
  assert ref['max_clusters'][0] > 8 and ref['max_clusters'][1] <= 8
  dec = _capi.Decoder(params)
  frames, offsets = oracle_lib.pack(seqs)
  for flags in (_capi.UIS_FLAG_RESIDENT, _capi.UIS_FLAG_STEPWISE):
    out = dec.decode(frames, offsets, 8, 1, 2, max_clusters=8, flags=flags)
    assert out['status'] == _capi.UIS_ERR_CLUSTER_CAP
    assert out['overflow'].tolist() == [1, 0, 1]
    assert np.array_equal(out['labels'][offsets[1]:offsets[2]], ref['labels'][1])
  model_args, _, inference_args = uisrnn_amd.parse_arguments([])
  inference_args.beam_size = 8
  inference_args.max_clusters = 8
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params)
  assert model.predict(seqs, inference_args) == [x.tolist() for x in ref['labels']]


@pytest.mark.parametrize('dim,hidden,threads', [(256, 512, '3'), (20, 24, '5'), (256, 512, '')])
def test_float64_utterances_through_uis_decode_f64(dim, hidden, threads, oracle_lib, monkeypatch):
  """uis_decode_f64 (the list of float64 arrays predict() receives, cast by the library's own
  threads chunk by chunk) gives bit for bit what uis_decode gives on the caller-cast float32
  frames: ragged lengths, empty utterances, several copy chunks, values that round in the cast."""
  if threads:
    monkeypatch.setenv('UIS_CAST_THREADS', threads)
  params = synth.tracker_params(dim, hidden, 1, seed=0)
  lengths = [300, 0, 431, 257, 1, 0, 390, 300] * 6   # 9474 frames: two copy chunks
  seqs, _ = synth.make_utterances(9461, len(lengths), [max(n, 1) for n in lengths], dim)
  rng = np.random.default_rng(5)
  seqs = [(s[:n] + 1e-9 * rng.standard_normal((n, dim))) for s, n in zip(seqs, lengths)]  # not exactly representable in f32
  frames = np.concatenate(seqs).astype(np.float32)
  offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
  dec = _capi.Decoder(params)
  want = dec.decode(frames, offsets, 10, 1, 2, want_beam_scores=True)
  got = dec.decode_f64(seqs, 10, 1, 2, want_beam_scores=True)
  assert got['status'] == want['status'] == 0
  assert np.array_equal(got['labels'], want['labels'])
  assert np.array_equal(_bits(got['beam_scores']), _bits(want['beam_scores']))
  # a second call with fewer frames reuses the staging buffer; nothing of the first call leaks in
  got2 = dec.decode_f64(seqs[:8], 10, 1, 2)
  want2 = dec.decode(frames[:offsets[8]], offsets[:9], 10, 1, 2)
  assert np.array_equal(got2['labels'], want2['labels'])
  assert np.array_equal(_bits(got2['scores']), _bits(want2['scores']))
  assert dec.decode_f64([], 10, 1, 2)['labels'].size == 0


def test_python_surface_and_demo_flow(tmp_path, oracle_lib):
  """uisrnn_amd.UISRNN.predict / parallel_predict / save+load, as the reference's demo uses them."""
  import subprocess
  import sys as _sys
  import uisrnn_amd
  model_args, _, inference_args = uisrnn_amd.parse_arguments([])
  model = uisrnn_amd.UISRNN(model_args)
  params = synth.tracker_params(256, 512, 1, seed=0)
  model.load_params(params)
  seqs, _ = synth.make_utterances(9000, 5, [60, 33, 1, 80, 45], 256)
  ref = oracle_lib.decode(params, seqs, 10, 1, 2, n_threads=4)
  got = model.predict(seqs, inference_args)
  assert got == [l.tolist() for l in ref['labels']]
  assert model.predict(seqs[0], inference_args) == ref['labels'][0].tolist()
  assert uisrnn_amd.parallel_predict(model, seqs, inference_args, num_processes=2) == got
  assert all(isinstance(v, int) for v in got[0])
  # checkpoint round trip in the reference's format keeps the predictions
  path = str(tmp_path / 'm.uisrnn')
  model.save(path)
  other = uisrnn_amd.UISRNN(model_args)
  other.load(path)
  assert other.predict(seqs, inference_args) == got
  # look_ahead through the Python surface, and the cluster-cap retry of the host layer
  inference_args.look_ahead = 2
  inference_args.beam_size = 5
  ref2 = oracle_lib.decode(params, seqs, 5, 2, 2, n_threads=4)
  assert model.predict(seqs, inference_args) == [l.tolist() for l in ref2['labels']]
  inference_args.look_ahead = 1
  inference_args.beam_size = 8
  inference_args.max_clusters = 2  # forces the retry loop (the data needs more)
  many, rng = _many_cluster_case()
  mseqs = [rng.standard_normal((30, 64)), rng.standard_normal((12, 64))]
  margs, _, _ = uisrnn_amd.parse_arguments(['--observation_dim', '64', '--rnn_hidden_size', '48'])
  mmodel = uisrnn_amd.UISRNN(margs)
  mmodel.load_params(many)
  refm = oracle_lib.decode(many, mseqs, 8, 1, 2)
  assert mmodel.predict(mseqs, inference_args) == [l.tolist() for l in refm['labels']]
  # the demo script end to end
  out = subprocess.run([_sys.executable, 'demo.py', '--test_data', str(tmp_path / 'none.npz')],
                       capture_output=True, text=True, cwd=str(tmp_path))
  assert out.returncode != 0  # missing file is an error, not a silent fallback
  root = __import__('os').path.dirname(__import__('os').path.dirname(__import__('os').path.abspath(__file__)))
  out = subprocess.run([_sys.executable, __import__('os').path.join(root, 'demo.py')],
                       capture_output=True, text=True, cwd=str(tmp_path))  # (output_result appends a file to the cwd)
  assert out.returncode == 0, out.stderr[-2000:]
  assert 'averaged accuracy' in out.stdout
  assert (tmp_path / 'layer_512_1_0.2_result.txt').exists()
  acc = float(out.stdout.split('averaged accuracy')[1].split(',')[0])
  assert acc > 0.97


def test_non_finite_input_empties_the_beam(oracle_lib):
  """A nan frame makes every candidate non-finite: no survivors, labels -1, like the oracle;
  the Python surface raises IndexError like the reference's beam_set[0] (uisrnn.py:561)."""
  import uisrnn_amd
  params = synth.tracker_params(256, 512, 1, seed=0)
  seqs, _ = synth.make_utterances(9500, 3, [20, 15, 10], 256)
  seqs[1][7, 3] = np.nan
  ref = oracle_lib.decode(params, seqs, 10, 1, 2)
  dec = _capi.Decoder(params)
  frames, offsets = oracle_lib.pack(seqs)
  out = dec.decode(frames, offsets, 10, 1, 2, want_beam_scores=True)
  assert out['status'] == 0
  for u in range(3):
    assert np.array_equal(out['labels'][offsets[u]:offsets[u + 1]], ref['labels'][u])
  assert (ref['labels'][1] == -1).all() and np.isinf(out['scores'][1])
  assert (ref['labels'][0] >= 0).all()
  model_args, _, inference_args = uisrnn_amd.parse_arguments([])
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params)
  with pytest.raises(IndexError):
    model.predict(seqs, inference_args)
  with pytest.raises(ValueError):   # the reference raises either, depending on the step (probes.json)
    model.predict(seqs, inference_args)
  assert model.predict([seqs[0], seqs[2]], inference_args) == [
      ref['labels'][0].tolist(), ref['labels'][2].tolist()]


def test_parallel_predict_worker_threads(oracle_lib):
  """parallel_predict shards over devices with one handle + thread each; on a one-GPU box the
  same device index is given twice/thrice to exercise exactly that path."""
  import uisrnn_amd
  model_args, _, inference_args = uisrnn_amd.parse_arguments([])
  model = uisrnn_amd.UISRNN(model_args)
  params = synth.tracker_params(256, 512, 1, seed=0)
  model.load_params(params)
  lengths = [70, 12, 45, 90, 33, 5, 64, 51, 20]
  seqs, _ = synth.make_utterances(9700, len(lengths), lengths, 256)
  want = [l.tolist() for l in oracle_lib.decode(params, seqs, 10, 1, 2, n_threads=4)['labels']]
  assert uisrnn_amd.parallel_predict(model, seqs, inference_args) == want
  assert uisrnn_amd.parallel_predict(model, seqs, inference_args, devices=[0, 0]) == want
  assert uisrnn_amd.parallel_predict(model, seqs, inference_args, devices=[0, 0, 0]) == want
  assert uisrnn_amd.parallel_predict(model, seqs[:1], inference_args, devices=[0, 0]) == want[:1]
  with pytest.raises(ValueError):
    uisrnn_amd.parallel_predict(model, [np.zeros((3, 5))], inference_args, devices=[0, 0])


def test_empty_inputs_through_the_c_abi():
  """No utterances / only empty utterances: no kernels to run, well-defined outputs."""
  params = synth.tracker_params(256, 512, 1, seed=0)
  dec = _capi.Decoder(params)
  out = dec.decode(np.zeros((0, 256), np.float32), np.zeros(1, np.int64), 10, 1, 2)
  assert out['status'] == 0 and out['labels'].size == 0 and out['scores'].size == 0
  out = dec.decode(np.zeros((0, 256), np.float32), np.zeros(4, np.int64), 10, 2, 2,
                   want_beam_scores=True)
  assert out['status'] == 0 and out['scores'].tolist() == [0.0, 0.0, 0.0]
  assert np.isinf(out['beam_scores']).all()
  # bad options are rejected, not executed
  lib = _capi.load_library()
  for kwargs in (dict(beam_size=0), dict(look_ahead=0), dict(test_iteration=0),
                 dict(beam_size=40000), dict(look_ahead=2000)):   # (round 5: beam 300 and look_ahead 9 are decoded)
    args = dict(beam_size=10, look_ahead=1, test_iteration=2)
    args.update(kwargs)
    with pytest.raises(_capi.HipLibraryError):
      dec.decode(np.zeros((2, 256), np.float32), np.array([0, 2], np.int64), **args)
  assert lib.uis_last_error()


def test_calculate_score_arrays_on_the_device(oracle_lib):
  """The device's FULL candidate arrays (UIS_FLAG_DEBUG_SCORES) against what the reference's
  _calculate_score returned (uisrnn/uisrnn.py:455-477; tests/golden/fn_scores.npz) and, bit for bit,
  against the oracle's -- on every path that scores candidates: the four look_ahead-1 selects and,
  for look_ahead >= 2, k_window's whole [beam, C, C] grid of a window (ragged last window and the
  +inf padding included), not only the survivors."""
  data = np.load(golden_util.GOLDEN_DIR + '/fn_scores.npz')
  checked = windows = 0
  for i in range(int(data['n_cases'])):
    name = str(data['case_{}'.format(i)][0])
    utt, keep, beam, look, tau, cmax = (int(v) for v in data['cfg_{}'.format(i)])
    ref = data['scores_{}'.format(i)]
    case = golden_util.load_trained(name) if name.startswith('trained_') else golden_util.load_case(name)
    seq = np.asarray(case['seqs'][utt], dtype=np.float64)[:keep]
    ora = oracle_lib.candidate_scores(case['params'], seq, beam, look, tau, cmax)
    dec = _capi.Decoder(case['params'])
    frames, offsets = oracle_lib.pack([seq])
    kmax = cmax - 1
    if look == 1:
      paths = [0, _capi.UIS_FLAG_STEPWISE, _capi.UIS_FLAG_OWNER_SELECT,
               _capi.UIS_FLAG_STEPWISE | _capi.UIS_FLAG_GENERIC_SELECT]
    else:
      paths = [0, _capi.UIS_FLAG_STEPWISE, _capi.UIS_FLAG_NO_DEDUP, _capi.UIS_FLAG_SMALL_TILES]
    n_win = (tau * keep + look - 1) // look
    for fl in paths:
      out = dec.decode(frames, offsets, beam, look, tau, max_clusters=kmax,
                       flags=fl | _capi.UIS_FLAG_DEBUG_SCORES)
      assert out['status'] == 0
      got = dec.debug_scores(n_win, 1, beam, kmax, look)[:, 0]
      assert got.shape == ref.shape
      assert np.array_equal(_bits(got), _bits(ora)), (name, fl)
      assert np.array_equal(np.isinf(got), np.isinf(ref))
      fin = np.isfinite(ref)
      np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-4)
      checked += 1
      windows += n_win if look > 1 else 0
  assert checked >= 16 + 6 and windows >= 3 * (5 + 8)


def test_level_capacity_names_the_utterances_and_keeps_the_others(oracle_lib, monkeypatch):
  """The Python surface on the level capacity (round 5).  A window whose live prefixes outgrow the default
  32768 hypotheses per level is no longer an error: predict() decodes the affected utterances again with eight
  times the room and returns the reference's labels for everybody (the oracle's, bit for bit).  Only a window
  beyond the largest capacity (524287 per level; lowered for this test) still ends in LookAheadWindowError,
  which names the utterances and carries the label lists of every other one -- nothing valid is thrown away."""
  import uisrnn_amd
  params, rng = _many_cluster_case()
  model_args, _, inference_args = uisrnn_amd.parse_arguments([])
  model_args.observation_dim = 64
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params)
  wild = rng.standard_normal((17, 64))                      # opens a cluster per frame
  calm = np.tile(rng.standard_normal((1, 64)), (9, 1)) + 0.01 * rng.standard_normal((9, 64))
  # beam 200, look_ahead 3: 200 * (K + 1) * (K + 2) prefixes -- past 32768 from K = 12 on
  inference_args.beam_size, inference_args.look_ahead, inference_args.test_iteration = 200, 3, 1
  inference_args.max_clusters = 30
  ref = oracle_lib.decode(params, [calm, wild], 200, 3, 1, n_threads=2)
  dec = model._get_decoder()  # pylint: disable=protected-access
  with pytest.raises(_capi.HipLibraryError, match='look-ahead window'):   # (the C ABI with too small a capacity says so)
    dec.decode(*oracle_lib.pack([calm, wild]), 200, 3, 1, max_clusters=30, level_cap=4096)
  assert dec.last_overflow()[1] == 2   # (bit 1: an intermediate level was full)
  inference_args.level_cap = 4096                             # (start the retries low: 4096 -> 32768 -> 262144)
  got = model.predict([calm, wild], inference_args)          # (the host layer retries the second one with more room)
  assert got == [ref['labels'][0].tolist(), ref['labels'][1].tolist()]
  inference_args.level_cap = 0
  assert model.predict([calm, wild], inference_args) == got   # (the default capacity: with or without a retry)
  out = dec.decode(*oracle_lib.pack([calm, wild]), 200, 3, 1, max_clusters=30, level_cap=262144, want_beam_scores=True)
  assert out['status'] == 0 and np.array_equal(_bits(out['beam_scores']), _bits(ref['beam_scores']))
  # the end of the retries (the largest capacity, lowered here so that the test stays small): the error names the
  # utterance in the caller's numbering and keeps the other one's labels (a one-frame utterance has no intermediate level)
  from uisrnn_amd import uisrnn as host
  monkeypatch.setattr(host, '_MAX_LEVEL_CAP', 4096)
  inference_args.level_cap = 4096
  one = rng.standard_normal((1, 64))
  with pytest.raises(uisrnn_amd.LookAheadWindowError) as info:
    model.predict([one, wild], inference_args)
  assert info.value.utterances == (1,)
  assert info.value.results[1] is None
  assert info.value.results[0] == oracle_lib.decode(params, [one], 200, 3, 1)['labels'][0].tolist()


def test_no_option_value_the_reference_takes_is_refused(oracle_lib):
  """Round 5 (the verdict's item 7): beam_size beyond the select kernels' 256, a cluster cap beyond their LDS
  budget and look_ahead beyond 8 are decoded -- by the window machinery, a launch per sub-step with the candidate
  lists in HBM (uis_stats.decode_kernel says 'stepwise') -- and agree with the oracle bit for bit.  The reference
  takes any of them (uisrnn/uisrnn.py:469-476,534-545: it enumerates every tuple)."""
  import uisrnn_amd
  rng = np.random.default_rng(77)
  params = weights.init_params(16, 8, 1, sigma2=0.3, transition_bias=0.4, crp_alpha=1.0, seed=5)
  # (a) beam 300, look_ahead 1 (and 2), ragged utterances incl. one frame
  seqs = [rng.standard_normal((n, 16)) for n in (13, 1, 7, 10)]
  frames, offsets = oracle_lib.pack(seqs)
  dec = _capi.Decoder(params)
  for beam, look, tau in ((300, 1, 2), (300, 2, 1), (700, 1, 1)):
    ref = oracle_lib.decode(params, seqs, beam, look, tau, n_threads=4)
    cap = int(ref['max_clusters'].max()) + look - 1
    out = dec.decode(frames, offsets, beam, look, tau, max_clusters=cap, want_beam_scores=True)
    assert out['status'] == 0 and out['stats']['decode_kernel'].startswith('stepwise'), out['stats']['decode_kernel']
    for u in range(len(seqs)):
      assert np.array_equal(out['labels'][offsets[u]:offsets[u + 1]], ref['labels'][u]), (beam, look, u)
    assert np.array_equal(_bits(out['beam_scores']), _bits(ref['beam_scores'])), (beam, look)
  # (b) a cluster cap the select kernels' LDS does not hold: beam 64, 200 clusters per hypothesis
  ref = oracle_lib.decode(params, seqs, 64, 1, 1, n_threads=4)
  out = dec.decode(frames, offsets, 64, 1, 1, max_clusters=200, want_beam_scores=True)
  assert out['status'] == 0 and np.array_equal(_bits(out['beam_scores']), _bits(ref['beam_scores']))
  assert np.array_equal(out['labels'], np.concatenate(ref['labels']))
  # (c) look_ahead 9: ONE window of nine frames from the empty beam -- 8! = 40320 prefixes on its last level (past the
  # default capacity: the C ABI takes it with level_cap, predict() gets there by its retry), 9! candidates pruned to 6
  nine = [rng.standard_normal((9, 16)), rng.standard_normal((4, 16))]
  ref = oracle_lib.decode(params, nine, 6, 9, 1, n_threads=2)
  out = dec.decode(*oracle_lib.pack(nine), 6, 9, 1, max_clusters=10, level_cap=65536, want_beam_scores=True)
  assert out['status'] == 0 and np.array_equal(_bits(out['beam_scores']), _bits(ref['beam_scores']))
  assert np.array_equal(out['labels'], np.concatenate(ref['labels']))
  model_args, _, inference_args = uisrnn_amd.parse_arguments([])
  model_args.observation_dim, model_args.rnn_hidden_size = 16, 8
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params)
  inference_args.beam_size, inference_args.look_ahead, inference_args.test_iteration = 6, 9, 1
  assert model.predict(nine, inference_args) == [l.tolist() for l in ref['labels']]
  inference_args.beam_size, inference_args.look_ahead = 300, 1
  assert model.predict(seqs, inference_args) == [l.tolist() for l in oracle_lib.decode(params, seqs, 300, 1, 1, n_threads=4)['labels']]


@pytest.mark.parametrize('beam,look,tau', [(300, 1, 2), (10, 4, 2), (40, 3, 1)], ids=['beam300_L1', 'beam10_L4', 'beam40_L3'])
def test_generic_window_path_at_a_real_model_size(beam, look, tau, oracle_lib):
  """Round 6 (the verdict's item 6): the window machinery -- the launch-per-sub-step form with candidate lists in HBM
  (uis_stats.decode_kernel 'stepwise...', what decodes whatever the one-launch shapes do not take) and, where it
  applies, the one-launch k_decode_big<WIN> -- at the BASELINE model's size:
  the checkpoint the reference trained (D 256 / H 512), 4 x 40 frames, beam 300 at look_ahead 1 and beam 10 / 40 at
  look_ahead 4 / 3, against the oracle bit for bit: labels, best scores, whole final beams (uisrnn/uisrnn.py:469-476,534-545)."""
  import os
  from uisrnn_amd import weights as wts
  params = wts.load_checkpoint(os.path.join(golden_util.GOLDEN_DIR, 'trained_d256.uisrnn'))
  seqs, _ = synth.make_utterances(26_000 + beam, 4, [40, 33, 40, 17], 256)
  ref = oracle_lib.decode(params, seqs, beam, look, tau, n_threads=4)
  frames, offsets = oracle_lib.pack(seqs)
  cap = max(int(ref['max_clusters'].max()) + look - 1, 4)
  dec = _capi.Decoder(params)
  # the default dispatch (beam 300: launch per step, k_window + k_wt_*; look_ahead 3 / 4 at these beams: the one-launch
  # window kernel's run-time instantiation) and the launch-per-sub-step window path demanded outright
  for flags, want in ((0, 'stepwise' if look == 1 else 'k_decode_big<WIN>'), (_capi.UIS_FLAG_STEPWISE, 'stepwise')):
    out = dec.decode(frames, offsets, beam, look, tau, max_clusters=cap, want_beam_scores=True, flags=flags)
    assert out['status'] == 0 and out['stats']['decode_kernel'].startswith(want), (flags, out['stats']['decode_kernel'])
    for u in range(len(seqs)):
      assert np.array_equal(out['labels'][offsets[u]:offsets[u + 1]], ref['labels'][u]), (flags, u)
    assert np.array_equal(_bits(out['scores']), _bits(ref['scores'])), flags
    assert np.array_equal(_bits(out['beam_scores']), _bits(ref['beam_scores'])), flags


def test_a_refused_decode_leaves_no_stale_flags_behind(oracle_lib):
  """uis_last_decode_info after a decode that was refused for its OPTIONS must not hand out the
  previous decode's arrays (a 100-utterance batch followed by a 1-utterance call with a refused look_ahead
  used to copy 100 flags into a buffer of one): the library reports the shape it holds
  (uis_last_decode_shape: 0 x 0) and the Python surface raises the clean error."""
  import uisrnn_amd
  params = synth.tracker_params(64, 256, 1, seed=2)
  seqs, _ = synth.make_utterances(4200, 100, 6, 64)
  model_args, _, inference_args = uisrnn_amd.parse_arguments([])
  model_args.observation_dim = 64
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params)
  inference_args.beam_size, inference_args.look_ahead, inference_args.test_iteration = 4, 2, 1
  want = [l.tolist() for l in oracle_lib.decode(params, seqs, 4, 2, 1, n_threads=8)['labels']]
  assert model.predict(seqs, inference_args) == want
  dec = model._get_decoder()  # pylint: disable=protected-access
  assert dec.last_overflow().shape == (100,)
  inference_args.look_ahead = 2000   # (an option value beyond the window records' fields: refused before it starts)
  with pytest.raises(_capi.HipLibraryError) as info:
    model.predict(seqs[:1], inference_args)
  assert info.value.status == _capi.UIS_ERR_UNSUPPORTED and not isinstance(info.value, uisrnn_amd.LookAheadWindowError)
  assert dec.last_overflow().shape == (0,)
  assert dec.last_overflow(3).tolist() == [0, 0, 0]
  inference_args.look_ahead = 2
  assert model.predict(seqs[:3], inference_args) == want[:3]


def test_two_handles_decode_concurrently_on_one_device(oracle_lib):
  """Two handles on device 0, driven from two host threads at once, both on the one-launch
  replicated-select kernel (UIS_FLAG_RESIDENT: REQUIRE it -- a fallback to the launch-per-step path
  would be an error here, not a silent success).  Each launch is cooperative and owns every CU, so
  two of them cannot be resident together: the runtime has to run them one after the other, not
  refuse or abort one.  This is what a launcher that folds several ranks onto one GPU would do."""
  import threading
  params = synth.tracker_params(256, 512, 1, seed=0)
  batches = [synth.make_utterances(5100 + 100 * k, 64, 40, 256)[0] for k in range(2)]
  refs = [oracle_lib.decode(params, b, 10, 1, 2, n_threads=8) for b in batches]
  decs = [_capi.Decoder(params, device=0) for _ in range(2)]
  errors, kernels = [], [set(), set()]

  def worker(k):
    try:
      frames, offsets = oracle_lib.pack(batches[k])
      for _ in range(6):
        out = decs[k].decode(frames, offsets, 10, 1, 2, flags=_capi.UIS_FLAG_RESIDENT, want_beam_scores=True)
        assert out['status'] == 0
        kernels[k].add(out['stats']['decode_kernel'])
        for u in range(len(batches[k])):
          assert np.array_equal(out['labels'][offsets[u]:offsets[u + 1]], refs[k]['labels'][u])
        assert np.array_equal(_bits(out['beam_scores']), _bits(refs[k]['beam_scores']))
    except BaseException as e:  # pylint: disable=broad-except
      errors.append((k, repr(e)))

  threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
  for t in threads:
    t.start()
  for t in threads:
    t.join()
  assert not errors, errors
  assert kernels == [{'k_decode_rs'}, {'k_decode_rs'}], kernels


def test_reference_probes_on_the_device():
  """tests/golden/probes.json on the DEVICE path: which probe yields labels and which an empty beam.

  The reference (uisrnn/uisrnn.py:531,546-549,561) raises ValueError / IndexError when its beam
  empties and, with a NaN in the LAST frame, returns a label list one frame short (numpy sorts NaN
  behind the +inf padding; DESIGN.md 1.1 -- a documented deviation: non-finite candidates are never
  selected here).  Pinned on every select path: finite probes give the reference's labels, every
  non-finite probe gives -1 labels from the C ABI and EmptyBeamError -- an instance of the type the
  reference raised -- from predict()."""
  import json
  import os
  import uisrnn_amd
  with open(os.path.join(golden_util.GOLDEN_DIR, 'probes.json')) as f:
    probes = json.load(f)
  case = golden_util.load_case('tiny_d16')
  params, seq = case['params'], np.asarray(case['seqs'][0], dtype=np.float64)
  dec = _capi.Decoder(params)
  m0, _ = dec.constants()
  model_args, _, inference_args = uisrnn_amd.parse_arguments([])
  model_args.observation_dim = params['observation_dim']
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params)
  inference_args.beam_size, inference_args.look_ahead, inference_args.test_iteration = 5, 1, 1

  def edit(row, col, value):
    q = seq.copy()
    q[row, col] = value
    return q
  inputs = {
      'clean': seq,
      'first_component_equals_m0_frame4': edit(4, 0, np.float64(m0[0])),
      'first_component_equals_m0_frame0': edit(0, 0, np.float64(m0[0])),
      'nan_mid_frame': edit(3, 2, np.nan),
      'nan_last_frame': edit(seq.shape[0] - 1, 2, np.nan),
      'inf_first_frame': edit(0, 0, np.inf),
  }
  paths = [0, _capi.UIS_FLAG_STEPWISE, _capi.UIS_FLAG_STEPWISE | _capi.UIS_FLAG_GENERIC_SELECT]
  for name, x in inputs.items():
    rec = probes[name]
    frames = x.astype(np.float32)
    offsets = np.array([0, x.shape[0]], dtype=np.int64)
    for fl in paths:
      out = dec.decode(frames, offsets, 5, 1, 1, flags=fl)
      assert out['status'] == 0
      if 'labels' in rec and name != 'nan_last_frame':
        assert out['labels'].tolist() == rec['labels'], (name, fl)
      else:
        assert set(out['labels'].tolist()) == {-1}, (name, fl)
    if 'labels' in rec and name != 'nan_last_frame':
      assert model.predict(x, inference_args) == rec['labels']
    else:
      with pytest.raises(uisrnn_amd.EmptyBeamError) as info:
        model.predict(x, inference_args)
      if 'raises' in rec:  # the reference's own exception type is one of EmptyBeamError's bases
        assert isinstance(info.value, {'ValueError': ValueError, 'IndexError': IndexError}[rec['raises']])
      else:                # nan_last_frame: the reference returned a list ONE FRAME SHORT (its accident)
        assert len(rec['labels']) == x.shape[0] - 1


def _decode_and_check(dec, params, seqs, beam, cap, oracle_lib, want_kernel, flags=0):
  """`cap` = max_clusters, or None: what the oracle's survivors needed (at least 4)."""
  ref = oracle_lib.decode(params, seqs, beam, 1, 2, n_threads=8)
  frames, offsets = oracle_lib.pack(seqs)
  if cap is None:
    cap = max(int(ref['max_clusters'].max()), 4)
  out = dec.decode(frames, offsets, beam, 1, 2, max_clusters=cap, flags=flags, want_beam_scores=True)
  assert out['status'] == 0 and not out['overflow'].any(), (out['status'], cap, int(ref['max_clusters'].max()))
  assert out['stats']['decode_kernel'] == want_kernel, out['stats']['decode_kernel']
  for u in range(len(seqs)):
    assert np.array_equal(out['labels'][offsets[u]:offsets[u + 1]], ref['labels'][u]), u
  assert np.array_equal(_bits(out['scores']), _bits(ref['scores']))
  assert np.array_equal(_bits(out['beam_scores']), _bits(ref['beam_scores']))
  return out


def test_replicated_select_shape_classes(oracle_lib):
  """Two of k_decode_rs's seven instantiations (uis_select_rs.hip; all of them: tests/test_gpu_instantiations.py), both
  at hidden size 512 / observation dim 256, named by the library itself (uis_stats.decode_kernel), against the oracle
  bit for bit: the base class and the class with the
  benchmark's beam / cluster cap as compile-time constants -- ragged batches, with and without row
  de-duplication, and with the one-launch decode REQUIRED (no silent fallback).  Beyond its limits
  (beam_size 17 .. 32, observation_dim 512, 9 .. 16 utterances per XCD) the owner-select kernel
  decodes, also under UIS_FLAG_REPLICATED_SELECT, which once asked for k_decode_rs classes there and
  is now accepted and ignored."""
  res = _capi.UIS_FLAG_RESIDENT
  rep = res | _capi.UIS_FLAG_REPLICATED_SELECT
  rng = np.random.default_rng(5)
  # D = 256: base (cap 12), the fixed-shape instantiation (beam 10, cap 16), beams 17 .. 32
  params = synth.tracker_params(256, 512, 1, seed=3)
  dec = _capi.Decoder(params)
  lens = [int(n) for n in rng.integers(1, 70, size=61)]
  seqs, _ = synth.make_utterances(8100, len(lens), lens, 256)
  _decode_and_check(dec, params, seqs, 10, 12, oracle_lib, 'k_decode_rs', res)
  _decode_and_check(dec, params, seqs, 10, 16, oracle_lib, 'k_decode_rs', res)
  _decode_and_check(dec, params, seqs, 10, 16, oracle_lib, 'k_decode_rs', res | _capi.UIS_FLAG_NO_DEDUP)
  _decode_and_check(dec, params, seqs[:23], 24, None, oracle_lib, 'k_decode_resident', rep)
  _decode_and_check(dec, params, seqs[:9], 32, None, oracle_lib, 'k_decode_resident', rep | _capi.UIS_FLAG_NO_DEDUP)
  _decode_and_check(dec, params, seqs[:40], 17, None, oracle_lib, 'k_decode_resident', rep)
  # 9 .. 16 utterances per XCD
  lens2 = [int(n) for n in rng.integers(1, 40, size=117)]
  seqs2, _ = synth.make_utterances(8700, len(lens2), lens2, 256)
  _decode_and_check(dec, params, seqs2, 10, 16, oracle_lib, 'k_decode_resident', rep)
  _decode_and_check(dec, params, seqs2[:65], 10, 16, oracle_lib, 'k_decode_resident', rep)
  _decode_and_check(dec, params, seqs2[:128 - 11], 8, 12, oracle_lib, 'k_decode_resident', rep | _capi.UIS_FLAG_NO_DEDUP)
  _decode_and_check(dec, params, seqs2, 10, 16, oracle_lib, 'k_decode_resident', res)
  # D = 512 (configs[4]: beam 20, cap 11), and a narrow beam on the same model
  # (the model the reference trained for that config: its survivors stay within the cap, as in bench.py)
  import os
  from uisrnn_amd import weights
  params5 = weights.load_checkpoint(os.path.join(golden_util.GOLDEN_DIR, 'trained_d512.uisrnn'))
  dec5 = _capi.Decoder(params5)
  seqs5, _ = synth.make_utterances(8300, 64, lens[:61] + [33, 20, 5], 512)
  _decode_and_check(dec5, params5, seqs5[:64], 20, 11, oracle_lib, 'k_decode_resident', rep)
  _decode_and_check(dec5, params5, seqs5[:30], 6, 16, oracle_lib, 'k_decode_resident', rep)
  _decode_and_check(dec5, params5, seqs5[:30], 20, 11, oracle_lib, 'k_decode_resident', rep | _capi.UIS_FLAG_NO_DEDUP)
  _decode_and_check(dec5, params5, seqs5[:30], 20, 11, oracle_lib, 'k_decode_resident', res)


def test_candidate_arrays_on_the_wide_select(oracle_lib):
  """UIS_FLAG_DEBUG_SCORES on beam 20 at observation_dim 512, the shape k_decode_resident decodes
  (its select_fast_body keeps the scores): every candidate score of every step equals the
  oracle's, bit for bit."""
  import os
  from uisrnn_amd import weights
  params = weights.load_checkpoint(os.path.join(golden_util.GOLDEN_DIR, 'trained_d512.uisrnn'))
  seq = synth.make_utterances(8400, 1, 14, 512)[0][0]
  beam, kmax, tau = 20, 11, 2
  ora = oracle_lib.candidate_scores(params, seq, beam, 1, tau, kmax + 1)
  dec = _capi.Decoder(params)
  frames, offsets = oracle_lib.pack([seq])
  out = dec.decode(frames, offsets, beam, 1, tau, max_clusters=kmax, flags=_capi.UIS_FLAG_DEBUG_SCORES | _capi.UIS_FLAG_RESIDENT)
  assert out['status'] == 0 and out['stats']['decode_kernel'] == 'k_decode_resident'
  got = dec.debug_scores(tau * seq.shape[0], 1, beam, kmax)[:, 0]
  assert np.array_equal(_bits(got), _bits(ora))


def test_small_models_decode_in_one_launch(oracle_lib):
  """k_decode_small (round 4): models the size of the reference's own tests -- hidden size 8 / 24,
  rnn_depth 1, 2 and 3, observation dims that are not multiples of 16 -- run their whole beam
  search in ONE launch, one workgroup per utterance, on the launch-per-step kernels' own tile
  function.  Named by the library, REQUIRED with UIS_FLAG_RESIDENT (no silent fallback), bit for
  bit the oracle's labels / scores / whole final beams, also against the launch-per-step path
  (UIS_FLAG_STEPWISE), with and without row de-duplication, wide beams, one-frame utterances
  (the fixtures hold empty ones), and the reference's recorded outputs of those fixtures."""
  res = _capi.UIS_FLAG_RESIDENT
  for name in ('tiny_d16', 'toy_d2_depth2', 'd20_h24_depth3'):
    case = golden_util.load_case(name)
    dec = _capi.Decoder(case['params'])
    frames, offsets = oracle_lib.pack(case['seqs'])
    for run in case['runs']:
      if run['look_ahead'] != 1:
        continue
      ref = oracle_lib.decode(case['params'], case['seqs'], run['beam_size'], 1, run['test_iteration'], n_threads=8)
      cap = max(int(ref['max_clusters'].max()), 4)
      outs = {}
      for fl in (res, res | _capi.UIS_FLAG_NO_DEDUP, _capi.UIS_FLAG_STEPWISE, 0):
        out = dec.decode(frames, offsets, run['beam_size'], 1, run['test_iteration'], max_clusters=cap, flags=fl,
                         want_beam_scores=True)
        assert out['status'] == 0
        assert out['stats']['decode_kernel'] == ('k_decode_small' if not fl & _capi.UIS_FLAG_STEPWISE else 'stepwise:k_dense'), (name, fl)
        for u in range(len(case['seqs'])):
          assert np.array_equal(out['labels'][offsets[u]:offsets[u + 1]], ref['labels'][u]), (name, fl, u)
          assert np.array_equal(out['labels'][offsets[u]:offsets[u + 1]], run['labels'][u]), (name, fl, u)  # the reference's own
        assert np.array_equal(_bits(out['beam_scores']), _bits(ref['beam_scores'])), (name, fl)
        outs[fl] = out
      assert outs[res]['stats']['rnn_rows'] == outs[_capi.UIS_FLAG_STEPWISE]['stats']['rnn_rows']
  # a wide beam (40 of at most 64: 40 x 6 = 240 candidates), many short utterances, a single frame, depth 2
  from uisrnn_amd import weights
  rng = np.random.default_rng(17)
  params = weights.init_params(33, 17, 2, sigma2=0.1, transition_bias=0.2, crp_alpha=1.0, seed=5)
  params['rnn_init_hidden'] = (0.2 * rng.standard_normal((2, 17))).astype(np.float32)
  cents = rng.standard_normal((3, 33))
  lens = [1, 7, 19, 30, 4] + [int(n) for n in rng.integers(1, 25, size=70)]
  seqs = [(cents[np.repeat(rng.integers(0, 3, size=n // 4 + 1), 4)[:n]] * 0.4 + 0.1 * rng.standard_normal((n, 33))) for n in lens]
  for beam, tau in ((4, 2), (40, 1)):
    out, _ = _compare(params, seqs, beam, 1, tau, oracle_lib, flags=res)
    assert out['stats']['decode_kernel'] == 'k_decode_small'
  # look_ahead >= 2 on small models: the same kernel with a sub-step of the window kernel as its select
  for beam, look, tau, n in ((4, 2, 2, 20), (3, 3, 1, 12), (12, 2, 1, 8)):
    out, _ = _compare(params, seqs[:n], beam, look, tau, oracle_lib, flags=res)
    assert out['stats']['decode_kernel'] == 'k_decode_small'
  case = golden_util.load_case('d32_lookahead3')
  dec = _capi.Decoder(case['params'])
  frames, offsets = oracle_lib.pack(case['seqs'])
  for run in case['runs']:
    out, _ = _compare(case['params'], case['seqs'], run['beam_size'], run['look_ahead'], run['test_iteration'],
                      oracle_lib, decoder=dec, flags=res)
    assert out['stats']['decode_kernel'] == 'k_decode_small'
    for u in range(len(case['seqs'])):
      assert np.array_equal(out['labels'][offsets[u]:offsets[u + 1]], run['labels'][u])  # the reference's own


@pytest.mark.parametrize('hidden', [256, 512])
def test_depth2_upper_layer_on_the_lds_weight_kernels(hidden, oracle_lib):
  """rnn_depth 2 at hidden size 256 / 512 with thousands of rnn rows per step (launch-per-step path, k_wt_*):
  the upper layer's input-side gates run on the wave-per-row-tile kernel too (k_wt_gru<.., UP>) -- same
  canonical sums as the split-K tiles, so the oracle is matched bit for bit."""
  from uisrnn_amd import weights
  params = weights.init_params(48, hidden, 2, sigma2=0.1, transition_bias=0.2, crp_alpha=1.0, seed=hidden)
  params['rnn_init_hidden'] = (0.2 * np.random.default_rng(1).standard_normal((2, hidden))).astype(np.float32)
  rng = np.random.default_rng(hidden + 1)
  cents = rng.standard_normal((3, 48))
  lens = [int(n) for n in rng.integers(1, 9, size=260)]
  seqs = [(cents[np.repeat(rng.integers(0, 3, size=n // 4 + 1), 4)[:n]] * 0.4 + 0.1 * rng.standard_normal((n, 48))) for n in lens]
  out, _ = _compare(params, seqs, 8, 1, 1, oracle_lib, flags=_capi.UIS_FLAG_STEPWISE)
  assert out['stats']['decode_kernel'] == 'stepwise:k_wt'


def test_predict_decodes_an_oversized_list_in_halves(monkeypatch, oracle_lib):
  """predict(list) when the list's decode state exceeds what the library accepts (UIS_ERR_OOM; the ceiling
  lowered through UIS_MAX_STATE_BYTES): the host layer splits the list, recursively, and the labels come
  back in the caller's order, identical to the unsplit decode's."""
  import uisrnn_amd
  model_args, _, inference_args = uisrnn_amd.parse_arguments([])
  model = uisrnn_amd.UISRNN(model_args)
  params = synth.tracker_params(256, 512, 1, seed=0)
  model.load_params(params)
  lens = [40, 12, 33, 1, 25, 18, 30, 7, 22, 15, 9]
  seqs, _ = synth.make_utterances(9100, len(lens), lens, 256)
  whole = model.predict(seqs, inference_args)
  assert model.last_stats['decode_kernel'].startswith('k_decode_')
  # one utterance's state: S = 10 * 16 + 10 slots x (256 + 512) floats = 522 KB: room for three
  monkeypatch.setenv('UIS_MAX_STATE_BYTES', str(3.5 * 170 * 768 * 4))
  split = model.predict(seqs, inference_args)
  assert split == whole
  ref = oracle_lib.decode(params, seqs, 10, 1, 2, n_threads=4)
  assert split == [l.tolist() for l in ref['labels']]
  monkeypatch.setenv('UIS_MAX_STATE_BYTES', '1000')  # not even one utterance fits: the library's error goes up
  with pytest.raises(_capi.HipLibraryError):
    model.predict(seqs[:2], inference_args)


@pytest.mark.parametrize('dim,hidden,depth', [(48, 256, 2), (256, 512, 2), (30, 100, 3), (200, 500, 2)])
def test_deep_models_decode_in_one_launch(dim, hidden, depth, oracle_lib):
  """rnn_depth >= 2 at the cluster kernels' shapes (hidden size 65 .. 256 / 385 .. 512 after padding):
  k_decode_deep -- k_decode_big's stages with the workgroup's weight slot refilled per stage, one more pair
  of stages per upper layer -- against the oracle and the launch-per-step path, bit for bit, ragged
  utterances, few and many (more than one per workgroup)."""
  from uisrnn_amd import weights
  params = weights.init_params(dim, hidden, depth, sigma2=0.1, transition_bias=0.2, crp_alpha=1.0, seed=dim + hidden)
  params['rnn_init_hidden'] = (0.2 * np.random.default_rng(2).standard_normal((depth, hidden))).astype(np.float32)
  rng = np.random.default_rng(dim * 7 + hidden)
  cents = rng.standard_normal((3, dim))
  lens = [19, 6, 25, 1, 13, 9, 22, 4, 16]
  seqs = [(cents[np.repeat(rng.integers(0, 3, size=n // 4 + 1), 4)[:n]] * 0.4 + 0.1 * rng.standard_normal((n, dim))) for n in lens]
  dec = _capi.Decoder(params)
  out, ref = _compare(params, seqs, 6, 1, 2, oracle_lib, decoder=dec)
  frames, offsets = oracle_lib.pack(seqs)
  cap = int(ref['max_clusters'].max()) + 1
  one = dec.decode(frames, offsets, 6, 1, 2, max_clusters=cap, flags=_capi.UIS_FLAG_RESIDENT)
  assert one['status'] == 0 and one['stats']['decode_kernel'] == 'k_decode_deep'
  # look_ahead 2 / 3 on the deep model: the same kernel with a window sub-step as its select stage
  _, ref2 = _compare(params, seqs[:5], 4, 2, 1, oracle_lib, decoder=dec)
  f5, o5 = oracle_lib.pack(seqs[:5])
  two = dec.decode(f5, o5, 4, 2, 1, max_clusters=int(ref2['max_clusters'].max()) + 2)
  assert two['status'] == 0 and two['stats']['decode_kernel'] == 'k_decode_deep'
  _compare(params, seqs[:3], 3, 3, 1, oracle_lib, decoder=dec)
  # CoreRNN.forward through every layer of the padded model
  x = rng.standard_normal(dim).astype(np.float32)
  h0 = rng.standard_normal((depth, hidden)).astype(np.float32)
  mean, hout = dec.rnn_step(x, h0)
  mean_o, hout_o = oracle_lib.rnn_step(params, x, h0)
  assert np.array_equal(_bits(mean), _bits(mean_o)) and np.array_equal(_bits(hout), _bits(hout_o))
  if hidden == 256:
    many = [seqs[i % len(seqs)][:6] for i in range(300)]
    f2, o2 = oracle_lib.pack(many)
    big = dec.decode(f2, o2, 4, 1, 1, max_clusters=cap, want_beam_scores=True)
    assert big['status'] == 0 and big['stats']['decode_kernel'] == 'k_decode_deep'
    step = dec.decode(f2, o2, 4, 1, 1, max_clusters=cap, want_beam_scores=True, flags=_capi.UIS_FLAG_STEPWISE)
    assert np.array_equal(big['labels'], step['labels'])
    assert np.array_equal(_bits(big['beam_scores']), _bits(step['beam_scores']))


@pytest.mark.parametrize('n_utt,n_frames,beam,want', [(64, 160, 10, 'k_decode_rs'), (23, 131, 7, 'k_decode_rs'), (300, 130, 10, 'k_decode_big<WS>'),
                                                      (100, 140, 10, 'k_decode_resident'), (40, 150, 20, 'k_decode_resident')])
def test_decode_in_two_launches_with_the_later_frames_travelling_behind_the_first(n_utt, n_frames, beam, want, oracle_lib, monkeypatch):
  """Round 5 (the verdict's item 4): a list of equal-length utterances given in HOST memory is decoded in two or more
  launches of the one-launch kernel -- the first slice of every utterance's frames travels and is projected, the first launch
  decodes the steps that need nothing else, the rest of the frames travel and are projected behind it, the second
  launch picks the beam state up (k_decode_rs / k_decode_big<WS>: DecodeState::resume; k_decode_resident: the global beam tables).  Bit for bit the single launch (UIS_NO_SPLIT=1), the
  launch-per-step path and the oracle, for every split point incl. the smallest and the largest, through the packed
  float32 entry and the float64 list (uis_decode_f64: the cast in the order the frames are needed)."""
  import os
  from uisrnn_amd import weights as wts
  dim = 512 if beam == 20 else 256   # (beam 20: the configs[4] shape -- the model the reference trained at D = 512, cap 11)
  cap = 11 if beam == 20 else 0
  params = wts.load_checkpoint(os.path.join(golden_util.GOLDEN_DIR, 'trained_d{}.uisrnn'.format(dim)))
  seqs, _ = synth.make_utterances(51_000 + n_utt, n_utt, n_frames, dim)
  frames, offsets = oracle_lib.pack(seqs)
  dec = _capi.Decoder(params)
  monkeypatch.setenv('UIS_SPLIT_MIN_MB', '0')   # (the smallest list here is 3 MB: below what the library spends a launch on)
  monkeypatch.setenv('UIS_NO_SPLIT', '1')
  one = dec.decode(frames, offsets, beam, 1, 2, max_clusters=cap, want_beam_scores=True)
  assert one['status'] == 0 and one['stats']['decode_kernel'] == want and one['stats']['decode_launches'] == 1
  monkeypatch.delenv('UIS_NO_SPLIT')
  for t1, launches in ((None, None), ('32', 2), ('33', 2), ('77', 2), (str(n_frames - 32), 2), ('40,81', 3), ('32,64,96', 4)):
    if t1 is None:   # (the library's own schedule: 32 frames first, then what travels during the launch before)
      monkeypatch.delenv('UIS_SPLIT_FRAMES', raising=False)
    else:
      monkeypatch.setenv('UIS_SPLIT_FRAMES', t1)
    for entry in ('f32', 'f64'):
      two = (dec.decode(frames, offsets, beam, 1, 2, max_clusters=cap, want_beam_scores=True) if entry == 'f32'
             else dec.decode_f64(seqs, beam, 1, 2, max_clusters=cap, want_beam_scores=True))
      assert two['status'] == 0 and (two['stats']['decode_launches'] == launches if launches else two['stats']['decode_launches'] >= 2), (t1, entry, two['stats']['decode_launches'])
      assert two['stats']['decode_kernel'] == want
      assert np.array_equal(two['labels'], one['labels']), (t1, entry)
      assert np.array_equal(_bits(two['scores']), _bits(one['scores'])), (t1, entry)
      assert np.array_equal(_bits(two['beam_scores']), _bits(one['beam_scores'])), (t1, entry)
      assert two['stats']['rnn_rows'] == one['stats']['rnn_rows'] and two['stats']['candidates'] == one['stats']['candidates']
  monkeypatch.delenv('UIS_SPLIT_FRAMES', raising=False)
  step = dec.decode(frames, offsets, beam, 1, 2, max_clusters=cap, want_beam_scores=True, flags=_capi.UIS_FLAG_STEPWISE)
  assert step['stats']['decode_launches'] == 0
  assert np.array_equal(step['labels'], one['labels']) and np.array_equal(_bits(step['beam_scores']), _bits(one['beam_scores']))
  sample = [0, n_utt // 2, n_utt - 1]
  ref = oracle_lib.decode(params, [seqs[u] for u in sample], beam, 1, 2, n_threads=3)
  for k, u in enumerate(sample):
    assert np.array_equal(one['labels'][offsets[u]:offsets[u + 1]], ref['labels'][k]), u
    assert np.array_equal(_bits(one['beam_scores'][u]), _bits(ref['beam_scores'][k])), u
  # a small ragged list keeps the single launch (worth it from 64 MB of frames on), and so does a small list of equal lengths
  monkeypatch.delenv('UIS_SPLIT_MIN_MB')
  tiny = dec.decode(*oracle_lib.pack(seqs[:2]), beam, 1, 2, max_clusters=cap)
  assert tiny['status'] == 0 and tiny['stats']['decode_launches'] == 1
  ragged = [s[:n_frames - (u % 3)] for u, s in enumerate(seqs)]
  out = dec.decode(*oracle_lib.pack(ragged), beam, 1, 2, max_clusters=cap)
  assert out['status'] == 0 and out['stats']['decode_launches'] == 1


def test_ragged_list_in_several_launches(oracle_lib, monkeypatch):
  """... and a ragged list of 64 MB of frames or more, given as float64 arrays, does take the several launches: the cast lays
  the staging block out slice after slice (one copy each), a kernel scatters a slice to the utterance-major frame stream,
  the projection's batches come from a table -- utterances shorter than the first slice, shorter than a later one, of one
  frame.  Bit for bit the single launch and (a sample) the oracle, float32 and float64 entries."""
  import os
  from uisrnn_amd import weights as wts
  params = wts.load_checkpoint(os.path.join(golden_util.GOLDEN_DIR, 'trained_d256.uisrnn'))
  n_utt = 300
  lens = [150 + (37 * u) % 140 for u in range(n_utt)]
  lens[0], lens[1], lens[2], lens[7] = 1, 20, 33, 289
  seqs, _ = synth.make_utterances(61_000, n_utt, lens, 256)
  assert sum(lens) * 256 * 4 >= 64e6
  frames, offsets = oracle_lib.pack(seqs)
  dec = _capi.Decoder(params)
  monkeypatch.setenv('UIS_NO_SPLIT', '1')
  one = dec.decode(frames, offsets, 10, 1, 2, want_beam_scores=True)
  assert one['status'] == 0 and one['stats']['decode_kernel'] == 'k_decode_big<WS>' and one['stats']['decode_launches'] == 1
  monkeypatch.delenv('UIS_NO_SPLIT')
  for cuts in (None, '32', '40,100,200'):
    if cuts is None:
      monkeypatch.delenv('UIS_SPLIT_FRAMES', raising=False)
    else:
      monkeypatch.setenv('UIS_SPLIT_FRAMES', cuts)
    for entry in ('f32', 'f64'):
      two = (dec.decode(frames, offsets, 10, 1, 2, want_beam_scores=True) if entry == 'f32'
             else dec.decode_f64(seqs, 10, 1, 2, want_beam_scores=True))
      # (the packed float32 entry keeps one launch for a ragged list: its slices would be a copy per utterance -- measured
      # slower; the float64 entry lays its staging block out slice after slice)
      assert two['status'] == 0 and (two['stats']['decode_launches'] >= 2) == (entry == 'f64'), (cuts, entry, two['stats']['decode_launches'])
      assert np.array_equal(two['labels'], one['labels']), (cuts, entry)
      assert np.array_equal(_bits(two['beam_scores']), _bits(one['beam_scores'])), (cuts, entry)
  sample = [0, 1, 2, 7, 150, 299]
  ref = oracle_lib.decode(params, [seqs[u] for u in sample], 10, 1, 2, n_threads=6)
  for k, u in enumerate(sample):
    assert np.array_equal(one['labels'][offsets[u]:offsets[u + 1]], ref['labels'][k]), u
    assert np.array_equal(_bits(one['beam_scores'][u]), _bits(ref['beam_scores'][k])), u


def test_look_ahead_launch_beyond_2_gb_of_cluster_states(oracle_lib):
  """Round 5 (the verdict's item 2): 1024 utterances at configs[2]'s beam 50 / look_ahead 2 hold 2.7 GB of hidden states;
  k_decode_big<WIN> addresses them through 4 GB buffer descriptors with unsigned offsets and stays ONE launch (rounds 2-4:
  four launches per sub-step beyond 2 GB).  Bit for bit the launch-per-sub-step path; a sample against the oracle."""
  import os
  from uisrnn_amd import weights as wts
  params = wts.load_checkpoint(os.path.join(golden_util.GOLDEN_DIR, 'trained_d256.uisrnn'))
  n_utt = 1024
  lens = [10 + (3 * u) % 9 for u in range(n_utt)]
  seqs, _ = synth.make_utterances(71_000, n_utt, lens, 256)
  frames, offsets = oracle_lib.pack(seqs)
  dec = _capi.Decoder(params)
  one = dec.decode(frames, offsets, 50, 2, 2, max_clusters=12, want_beam_scores=True)
  assert one['status'] == 0 and one['stats']['decode_kernel'] == 'k_decode_big<WIN>', one['stats']['decode_kernel']
  step = dec.decode(frames, offsets, 50, 2, 2, max_clusters=12, want_beam_scores=True, flags=_capi.UIS_FLAG_STEPWISE)
  assert step['stats']['decode_kernel'].startswith('stepwise')
  assert np.array_equal(one['labels'], step['labels'])
  assert np.array_equal(_bits(one['beam_scores']), _bits(step['beam_scores']))
  sample = [0, 511, 1000, 1023]   # (the last utterances' states lie beyond 2 GB)
  ref = oracle_lib.decode(params, [seqs[u] for u in sample], 50, 2, 2, n_threads=4)
  for k, u in enumerate(sample):
    assert np.array_equal(one['labels'][offsets[u]:offsets[u + 1]], ref['labels'][k]), u
    assert np.array_equal(_bits(one['beam_scores'][u]), _bits(ref['beam_scores'][k])), u
