"""k_decode_rs's row list and per-step bookkeeping at their edges, against the CPU oracle, exact.

The step's row list is built from eight per-slot row counts (one byte each, a wave's first row and the step's total are
byte sums of that word) and the decode statistics are one 16-byte update per step per utterance; this file holds both to
the oracle where they can go wrong:

* row counts per XCD on both sides of the row-tile edges 16, 32 and 48 (beyond 48 the dense stages take a second pass):
  one, three and seven or eight utterances per XCD.  With UIS_FLAG_NO_DEDUP every winner is a row, so a slot with a full
  beam emits exactly beam_size rows and the counts are known in advance (printed below as a histogram, and asserted to
  reach every tile count); with de-duplication -- the product's path -- the counts are whatever the model decides and
  the mean is printed;
* waves without rows among waves with some: ragged lengths (slots end one by one), one utterance of three frames,
  XCDs that hold seven utterances beside XCDs that hold eight;
* stop and resume: the same list in two launches, cut where every slot is busy; the statistics are the one launch's;
* UIS_FLAG_DEBUG_SCORES on the smallest list: every candidate score of every step is the oracle's.

Statistics: rnn_rows_nodedup (one per winner), candidates and the largest cluster count have an oracle counterpart;
rnn_rows (after de-duplication) has none and is held to the launch-per-step path, which shares no code with the row list.
"""

import os

import numpy as np
import pytest

import golden_util
from uisrnn_amd import _capi, synth, weights

pytestmark = pytest.mark.gpu

RS_GENERIC, RS_FIXED = 1, 2   # uis_stats.decode_kernel_code bits 16..23
N_CLUSTERS = 8                # XCDs of a whole MI355X: utterance u is slot u // 8 of cluster u % 8
LONG, SHORT = 0, 5            # utterance LONG has 130 frames (a list has to reach 128 to be split), SHORT has 3


def _lengths(n_utt):
  return [130 if u == LONG else 3 if u == SHORT else 40 + (7 * u) % 21 for u in range(n_utt)]


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


MODELS = {
    # the fixed-shape class k_decode_rs<512, 256, 10, 16> on the trained D 256 / H 512 model
    'fixed': dict(dim=256, beam=10, cap=16, kind=RS_FIXED),
    # beam_size / max_clusters as run-time values: k_decode_rs<256, 128>
    'generic': dict(dim=128, beam=5, cap=16, kind=RS_GENERIC),
}


def _params(name):
  if name == 'fixed':
    return weights.load_checkpoint(os.path.join(golden_util.GOLDEN_DIR, 'trained_d256.uisrnn'))
  return synth.tracker_params(128, 256, 1, seed=81)


@pytest.fixture(scope='module')
def world(oracle_lib):
  """Per model: its parameters, 59 utterances (clusters 0 .. 2 hold eight, clusters 3 .. 7 seven) and a cache of oracle
  decodes of the list's prefixes -- each computed once, shared by the tests, never changed."""
  out = {}
  for name, spec in MODELS.items():
    params = _params(name)
    assert params['observation_dim'] == spec['dim']
    seqs, _ = synth.make_utterances(81_000 + spec['dim'], 59, _lengths(59), spec['dim'])
    out[name] = dict(spec, params=params, seqs=seqs, refs={})
  def ref(name, n_utt):
    w = out[name]
    if n_utt not in w['refs']:
      w['refs'][n_utt] = oracle_lib.decode(w['params'], w['seqs'][:n_utt], w['beam'], 1, 1, n_threads=16)
      assert int(w['refs'][n_utt]['max_clusters'].max()) <= w['cap'], 'the list outgrows the cap: not a case for this test'
    return w['refs'][n_utt]
  out['ref'] = ref
  return out


def _check(out, ref, spec, launches=1):
  assert out['status'] == 0
  assert out['stats']['decode_kernel'] == 'k_decode_rs', out['stats']['decode_kernel']
  assert (out['stats']['decode_kernel_code'] >> 16) & 0xff == spec['kind'], hex(out['stats']['decode_kernel_code'])
  assert out['stats']['decode_launches'] == launches
  assert not out['overflow'].any()
  assert np.array_equal(out['labels'], np.concatenate(ref['labels']))
  assert np.array_equal(_bits(out['scores']), _bits(ref['scores']))
  assert np.array_equal(_bits(out['beam_scores']), _bits(ref['beam_scores']))
  assert out['stats']['rnn_rows_nodedup'] == ref['rnn_calls']
  assert out['stats']['candidates'] == ref['candidates']
  assert out['stats']['max_clusters_seen'] == int(ref['max_clusters'].max())


def _full_beam_rows(lens, beam):
  """Rows per (step, cluster) of a list whose every slot emits beam_size rows from step 3 on (UIS_FLAG_NO_DEDUP, beam_size
  at most 10: see the test)."""
  rows = []
  for c in range(N_CLUSTERS):
    mine = [n for u, n in enumerate(lens) if u % N_CLUSTERS == c]
    rows += [beam * sum(1 for n in mine if n > s) for s in range(3, max(mine))]
  return np.array([r for r in rows if r > 0])


@pytest.mark.parametrize('n_utt', [8, 24, 59], ids=['one_per_xcd', 'three_per_xcd', 'seven_or_eight_per_xcd'])
@pytest.mark.parametrize('name', ['fixed', 'generic'])
def test_row_counts_across_the_tile_edges(name, n_utt, world, oracle_lib):
  w = world[name]
  ref = world['ref'](name, n_utt)
  lens = _lengths(n_utt)
  frames, offsets = oracle_lib.pack(w['seqs'][:n_utt])
  dec = _capi.Decoder(w['params'])
  try:
    one = dec.decode(frames, offsets, w['beam'], 1, 1, max_clusters=w['cap'], want_beam_scores=True)
    step = dec.decode(frames, offsets, w['beam'], 1, 1, max_clusters=w['cap'], flags=_capi.UIS_FLAG_STEPWISE)
    raw = dec.decode(frames, offsets, w['beam'], 1, 1, max_clusters=w['cap'], want_beam_scores=True,
                     flags=_capi.UIS_FLAG_NO_DEDUP)
  finally:
    dec.close()
  _check(one, ref, w)
  _check(raw, ref, w)
  assert step['status'] == 0 and step['stats']['decode_kernel'].startswith('stepwise')
  assert one['stats']['rnn_rows'] == step['stats']['rnn_rows']
  steps_x_clusters = sum(max(n for u, n in enumerate(lens) if u % N_CLUSTERS == c) for c in range(min(N_CLUSTERS, n_utt)))
  print('{} x {}: {:.1f} rows per step and XCD with de-duplication'.format(
      name, n_utt, one['stats']['rnn_rows'] / steps_x_clusters))
  # without de-duplication every winner is a row, and the beam is full from step 3 on: the counts are known
  assert raw['stats']['rnn_rows'] == raw['stats']['rnn_rows_nodedup'] == ref['rnn_calls']
  # (a hypothesis with K clusters has K + 1 candidates: one at step 0, two at step 1, 2 + 3 at step 2, ten or more from
  # step 3 on -- 1, 2, min(beam_size, 5), then beam_size winners per step, which the oracle's count confirms to the row)
  assert ref['rnn_calls'] == sum(min(w['beam'], (1, 2, 5)[s] if s < 3 else w['beam']) for n in lens for s in range(n))
  full = _full_beam_rows(lens, w['beam'])
  tiles = (full + 15) // 16
  print('{} x {}: rows per step and XCD without de-duplication, histogram by row tiles: {}'.format(
      name, n_utt, {int(t): int((tiles == t).sum()) for t in np.unique(tiles)}))
  if n_utt == 8:
    assert set(np.unique(tiles)) == {1}                         # below 16
  elif n_utt == 24:
    assert {1, 2} <= set(np.unique(tiles)) if w['beam'] == 10 else set(np.unique(tiles)) == {1}   # 30 / 20 / 10, or 15 / 10 / 5
  elif w['beam'] == 10:
    assert {1, 2, 3, 4, 5} <= set(np.unique(tiles))            # 80 and 70 rows down to 10: a second pass beyond 48
  else:
    assert {1, 2, 3} <= set(np.unique(tiles))                  # 40 rows down to 5


@pytest.mark.parametrize('name', ['fixed', 'generic'])
def test_stop_and_resume_keeps_the_statistics(name, world, monkeypatch):
  """Two launches, cut at frame 37: every slot but the three-frame one is busy there (seven or eight utterances per XCD),
  the second launch picks up the row counts of the first one's last step and the statistics it had gathered."""
  w = world[name]
  ref = world['ref'](name, 59)
  seqs = w['seqs']
  monkeypatch.setenv('UIS_SPLIT_MIN_MB', '0')
  monkeypatch.delenv('UIS_POISON_WORKSPACE', raising=False)
  dec = _capi.Decoder(w['params'])
  try:
    monkeypatch.setenv('UIS_NO_SPLIT', '1')
    one = dec.decode_f64(seqs, w['beam'], 1, 1, max_clusters=w['cap'], want_beam_scores=True)
    monkeypatch.delenv('UIS_NO_SPLIT')
    monkeypatch.setenv('UIS_SPLIT_FRAMES', '37')
    two = dec.decode_f64(seqs, w['beam'], 1, 1, max_clusters=w['cap'], want_beam_scores=True)
  finally:
    dec.close()
  _check(one, ref, w)
  _check(two, ref, w, launches=2)
  for key in ('rnn_rows', 'rnn_rows_nodedup', 'candidates', 'max_clusters_seen'):
    assert two['stats'][key] == one['stats'][key], key


def test_debug_scores_at_every_step(world, oracle_lib):
  """UIS_FLAG_DEBUG_SCORES on three short utterances of the fixed-shape class: the flag is tested once per step and the
  array's address is read behind it -- every step's scores have to be there."""
  w = world['fixed']
  n_utt, n_frames = 3, 12
  seqs = [s[:n_frames] for s in w['seqs'][1:1 + n_utt]]
  frames, offsets = oracle_lib.pack(seqs)
  dec = _capi.Decoder(w['params'])
  try:
    out = dec.decode(frames, offsets, w['beam'], 1, 1, max_clusters=w['cap'], flags=_capi.UIS_FLAG_DEBUG_SCORES)
    assert out['status'] == 0 and out['stats']['decode_kernel'] == 'k_decode_rs'
    assert (out['stats']['decode_kernel_code'] >> 16) & 0xff == RS_FIXED
    got = dec.debug_scores(n_frames, n_utt, w['beam'], w['cap'])
  finally:
    dec.close()
  for u, seq in enumerate(seqs):
    want = oracle_lib.candidate_scores(w['params'], seq, w['beam'], 1, 1, w['cap'] + 1)
    assert got[:, u].shape == want.shape
    assert np.array_equal(_bits(got[:, u]), _bits(want)), u
    assert np.isfinite(want[-1]).any()   # (the last step has scores: nothing stopped early)
