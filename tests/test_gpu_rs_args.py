"""k_decode_rs on its compact argument block (RsArgs): one buffer descriptor for the decode state, 32-bit offsets for the
frame stream, the rank's bias slices in LDS.  Every case decodes through k_decode_rs (asserted through
uis_stats.decode_kernel) and is compared bit for bit -- labels, scores, every beam score -- with the launch-per-step path
(UIS_FLAG_STEPWISE), which shares none of that addressing."""

import numpy as np
import pytest

from uisrnn_amd import _capi, synth

pytestmark = pytest.mark.gpu


def _bits(a):
  return np.ascontiguousarray(a).view(np.uint32)


RS_GENERIC, RS_FIXED = 1, 2   # uis_stats.decode_kernel bits 16..23: which k_decode_rs instantiation ran


def _rs_against_stepwise(dec, seqs, oracle_lib, beam, cap, kind, launches=1, tau=2):
  frames, offsets = oracle_lib.pack(seqs)
  rs = dec.decode(frames, offsets, beam, 1, tau, max_clusters=cap, want_beam_scores=True)
  assert rs['status'] == 0
  assert rs['stats']['decode_kernel'] == 'k_decode_rs', rs['stats']['decode_kernel']
  assert (rs['stats']['decode_kernel_code'] >> 16) & 0xff == kind, hex(rs['stats']['decode_kernel_code'])
  assert rs['stats']['decode_launches'] == launches, rs['stats']['decode_launches']
  step = dec.decode(frames, offsets, beam, 1, tau, max_clusters=cap, want_beam_scores=True, flags=_capi.UIS_FLAG_STEPWISE)
  assert step['status'] == 0 and step['stats']['decode_kernel'].startswith('stepwise')
  assert np.array_equal(rs['labels'], step['labels'])
  assert np.array_equal(_bits(rs['scores']), _bits(step['scores']))
  assert np.array_equal(_bits(rs['beam_scores']), _bits(step['beam_scores']))
  assert rs['stats']['rnn_rows'] == step['stats']['rnn_rows'] and rs['stats']['candidates'] == step['stats']['candidates']
  return rs


def test_fixed_shape_class(oracle_lib):
  """observation_dim 256, hidden 512, beam 10, cap 16: k_decode_rs<512, 256, 10, 16>; 64 utterances = eight per XCD,
  every wave of a workgroup decides one."""
  params = synth.tracker_params(256, 512, 1, seed=71)
  seqs, _ = synth.make_utterances(71_000, 64, [60] * 64, 256)
  _rs_against_stepwise(_capi.Decoder(params), seqs, oracle_lib, 10, 16, RS_FIXED)


@pytest.mark.parametrize('dim,hidden,beam,cap', [(256, 512, 8, 12), (128, 256, 10, 16), (128, 128, 5, 20)])
def test_generic_instantiations(dim, hidden, beam, cap, oracle_lib):
  """beam_size / max_clusters as run-time values (k_decode_rs<Hp, Dp>): the LDS layout is computed, not folded."""
  params = synth.tracker_params(dim, hidden, 1, seed=72 + beam)
  seqs, _ = synth.make_utterances(72_000 + dim, 24, [40 + (u % 3) for u in range(24)], dim)
  _rs_against_stepwise(_capi.Decoder(params), seqs, oracle_lib, beam, cap, RS_GENERIC)


def test_padded_model(oracle_lib):
  """hidden 300 (embedded in the 512-wide kernels) and an observation dim that is not a multiple of 16: the padded
  features stay zero through the buffer-addressed stores, the bias slices in LDS carry the padding's zeros."""
  params = synth.tracker_params(72, 300, 1, seed=73)
  seqs, _ = synth.make_utterances(73_000, 20, [35 + (3 * u) % 11 for u in range(20)], 72)
  _rs_against_stepwise(_capi.Decoder(params), seqs, oracle_lib, 10, 16, RS_GENERIC)


def test_two_launches_at_an_odd_boundary(oracle_lib, monkeypatch):
  """UIS_SPLIT_FRAMES=77: the second launch picks the beam state up from the hand-over block and the partial sums of
  the first launch's last step from the block the descriptor names."""
  params = synth.tracker_params(256, 512, 1, seed=74)
  seqs, _ = synth.make_utterances(74_000, 16, [150] * 16, 256)
  monkeypatch.setenv('UIS_SPLIT_MIN_MB', '0')
  monkeypatch.setenv('UIS_SPLIT_FRAMES', '77')
  _rs_against_stepwise(_capi.Decoder(params), seqs, oracle_lib, 10, 16, RS_FIXED, launches=2)


def test_ragged_list(oracle_lib):
  """Utterances of very different lengths, one of a single frame: slots go idle one by one while the others step on."""
  params = synth.tracker_params(256, 512, 1, seed=75)
  lens = [1, 2, 90, 17, 64, 33, 5, 120, 48, 77, 3, 101, 29, 64, 80, 12, 55, 9, 140, 41]
  seqs, _ = synth.make_utterances(75_000, len(lens), lens, 256)
  _rs_against_stepwise(_capi.Decoder(params), seqs, oracle_lib, 10, 16, RS_FIXED)


def test_without_the_arena(oracle_lib, monkeypatch):
  """UIS_NO_ARENA=1: every buffer its own allocation, except the stretch k_decode_rs addresses through one descriptor --
  the decode stays on k_decode_rs."""
  params = synth.tracker_params(256, 512, 1, seed=76)
  seqs, _ = synth.make_utterances(76_000, 12, [30 + u for u in range(12)], 256)
  monkeypatch.setenv('UIS_NO_ARENA', '1')
  _rs_against_stepwise(_capi.Decoder(params), seqs, oracle_lib, 10, 16, RS_FIXED)
