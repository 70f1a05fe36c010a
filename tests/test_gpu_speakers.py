"""uis_score_speakers / UISRNN.score_speakers on the GPU: every speaker's per-frame loss along a labeling.

1. the CPU restatement (tests/speakers_ref.py), bit for bit, on five model shapes and six kinds of labeling scored as
   one ragged batch;
2. identity 1: the chosen column is score_labels' per-frame loss, the scores are score_labels' scores;
3. identity 2: along a greedy decode's labels, float32(cum + rows) is the decode's own candidate array
   (UIS_FLAG_DEBUG_SCORES);
4. behaviour: width, sessions, the last decode's state, batch independence, poisoned workspace, what the call leaves
   behind for uis_score_labels and a primed session.
"""

import functools
import os

import numpy as np
import pytest

import forced_ref
import golden_util
import speakers_ref
import uisrnn_amd
from oracle import oracle
from uisrnn_amd import _capi, synth, weights

pytestmark = pytest.mark.gpu

MODELS = ('toy_d2_depth2', 'd20_h24_depth3', 'tracker_d64_h300', 'trained_d256', 'trained_d512')
WORDS = ('ffffffff', '7f7f7f7f', '80000000')   # test_gpu_poison.py's
KNOB = 'UIS_POISON_WORKSPACE'


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _params(model):
  if model.startswith('trained_'):
    return weights.load_checkpoint(os.path.join(golden_util.GOLDEN_DIR, model + '.uisrnn'))
  return golden_util.load_case(model)['params']


@functools.lru_cache(maxsize=None)
def _batch(model):
  """The ragged batch of one model: (seqs, labels, reference scores, reference rows), the reference computed once.

  greedy: the labels of a beam 1 decode; revisiting: 18 clusters that keep being returned to (more candidates than a
  workgroup has waves, and than 16); one_cluster: width 2, every prior after the first lp_stay; all_new: chains of
  length 1; invalid: K + 1 at frame 20; an empty and a one-frame utterance.  The order makes the chains' ranks
  (longest first) differ from their (utterance, cluster) order."""
  params = _params(model)
  dim = int(params['observation_dim'])
  lens = {'greedy': 48, 'revisiting': 44, 'one_cluster': 30, 'all_new': 12, 'invalid': 40, 'empty': 0, 'one_frame': 1}
  seqs = [synth.make_utterance(9100 + i, max(n, 1), dim)[0][:n] for i, n in enumerate(lens.values())]
  labels = [oracle.decode(params, [seqs[0]], 1, 1, 1)['labels'][0], speakers_ref.revisiting(44),
            speakers_ref.one_cluster(30), speakers_ref.all_new(12), speakers_ref.invalid_at(40), np.zeros(0, np.int32),
            np.zeros(1, np.int32)]
  scores, rows = speakers_ref.rows(params, seqs, labels)
  return tuple(lens), seqs, labels, scores, rows


def _cat(labels):
  return np.concatenate(labels).astype(np.int32)


def _check_batch(dec, model, what):
  names, seqs, labels, want_scores, want_rows = _batch(model)
  frames, offsets = oracle.pack(seqs)
  width = max(r.shape[1] for r in want_rows)
  assert width == 19
  scores, rows = dec.score_speakers(frames, offsets, _cat(labels), width)
  assert rows.shape == (int(offsets[-1]), width) and rows.dtype == np.float32
  assert np.array_equal(_bits(scores), _bits(want_scores)), (what, scores, want_scores)
  for u, name in enumerate(names):
    got = rows[offsets[u]:offsets[u + 1]]
    w = want_rows[u].shape[1]
    assert np.array_equal(_bits(got[:, :w]), _bits(want_rows[u])), (what, name)
    assert np.all(np.isposinf(got[:, w:])), (what, name)
  return scores, rows


@pytest.mark.parametrize('model', MODELS)
def test_rows_match_the_restatement(model):
  names, _, labels, want_scores, want_rows = _batch(model)
  dec = _capi.Decoder(_params(model), 0)
  try:
    _check_batch(dec, model, model)
  finally:
    dec.close()
  # what the batch is meant to exercise
  by = dict(zip(names, want_rows))
  assert by['revisiting'].shape == (44, 19) and by['one_cluster'].shape == (30, 2) and by['all_new'].shape == (12, 13)
  assert np.all(np.isposinf(by['invalid'][20:])) and np.all(np.isfinite(by['invalid'][:20, 0]))
  assert by['empty'].shape == (0, 1) and by['one_frame'].shape == (1, 2)
  assert np.isposinf(want_scores[names.index('invalid')]) and want_scores[names.index('empty')] == 0.0
  assert labels[0].shape == (48,)


def _truth_batch(n_utt, n_frames, seed):
  seqs, truth = synth.make_utterances(seed, n_utt, n_frames, 256)
  return seqs, [forced_ref.first_appearance(t.tolist()) for t in truth]


def test_chosen_column_is_score_labels():
  """Identity 1 on 8 x 60 frames of trained_d256: rows[t, c_t] == frame_losses_out[t], scores == score_labels'."""
  seqs, labels = _truth_batch(8, 60, 9200)
  frames, offsets = oracle.pack(seqs)
  flat = _cat(labels)
  dec = _capi.Decoder(_params('trained_d256'), 0)
  try:
    want_scores, want = dec.score_labels(frames, offsets, flat, want_frame_losses=True)
    width = int(flat.max()) + 2
    scores, rows = dec.score_speakers(frames, offsets, flat, width)
  finally:
    dec.close()
  assert np.array_equal(_bits(rows[np.arange(flat.shape[0]), flat]), _bits(want))
  assert np.array_equal(_bits(scores), _bits(want_scores))
  assert np.all(np.isfinite(want))


@pytest.mark.parametrize('model', ['trained_d256', 'toy_d2_depth2'])
def test_rows_are_the_decode_candidate_scores(model):
  """Identity 2 on the device: the greedy decode's labels and its candidate array under UIS_FLAG_DEBUG_SCORES."""
  params = _params(model)
  seq = synth.make_utterance(9300, 60, int(params['observation_dim']))[0]
  frames, offsets = oracle.pack([seq])
  kmax = 8
  dec = _capi.Decoder(params, 0)
  try:
    out = dec.decode(frames, offsets, 1, 1, 1, max_clusters=kmax, flags=_capi.UIS_FLAG_DEBUG_SCORES)
    assert out['status'] == 0
    want = dec.debug_scores(60, 1, 1, kmax)[:, 0, 0]
    labels = out['labels']
    assert int(labels.max()) + 1 < kmax  # (the cap was never in the way of a new speaker)
    scores, rows = dec.score_speakers(frames, offsets, labels, kmax + 1)
  finally:
    dec.close()
  assert np.array_equal(_bits(speakers_ref.candidates(rows, labels)), _bits(want))
  assert np.array_equal(np.isposinf(rows), np.isposinf(want))
  assert _bits(scores[0]) == _bits(out['scores'][0])


def test_width_sessions_and_the_last_decode():
  seqs, labels = _truth_batch(2, 40, 9400)
  frames, offsets = oracle.pack(seqs)
  flat = _cat(labels)
  need = max(int(l.max()) + 2 for l in labels)
  dec = _capi.Decoder(_params('trained_d256'), 0)
  try:
    decoded = dec.decode(frames, offsets, 4, 1, 1)
    nbest = dec.last_nbest(4)
    _, rows = dec.score_speakers(frames, offsets, flat, need)
    # a wider table: +inf in the extra columns, no other bit changes
    _, wide = dec.score_speakers(frames, offsets, flat, need + 5)
    assert np.array_equal(_bits(wide[:, :need]), _bits(rows)) and np.all(np.isposinf(wide[:, need:]))
    # one column too few: refused with a message, and the handle goes on working
    for bad in (need - 1, 0, -3):
      with pytest.raises(_capi.HipLibraryError, match='width') as err:
        dec.score_speakers(frames, offsets, flat, bad)
      assert err.value.status == _capi.UIS_ERR_INVALID_ARG
    _, again = dec.score_speakers(frames, offsets, flat, need)
    assert np.array_equal(_bits(again), _bits(rows))
    # into the caller's array
    mine = np.full((80, need), np.nan, dtype=np.float32)
    _, filled = dec.score_speakers(frames, offsets, flat, need, losses_out=mine)
    assert filled is mine and np.array_equal(_bits(mine), _bits(rows))
    with pytest.raises(ValueError, match='losses_out'):
      dec.score_speakers(frames, offsets, flat, need, losses_out=np.zeros((80, need + 1), np.float32))
    # refused while a session is open
    dec.stream_begin(1, 4, 100)
    try:
      with pytest.raises(_capi.HipLibraryError, match='streaming session is open'):
        dec.score_speakers(frames, offsets, flat, need)
    finally:
      dec.stream_end()
    # the last decode's results are still there
    after = dec.last_nbest(4)
    assert all(np.array_equal(a, b) for a, b in zip(after['labels'], nbest['labels']))
    assert np.array_equal(_bits(after['scores']), _bits(nbest['scores'])) and np.array_equal(after['counts'], nbest['counts'])
    assert np.array_equal(after['labels'][0][0], decoded['labels'][:40])
  finally:
    dec.close()


def test_batch_independence():
  """An utterance's rows do not depend on what it is scored with: alone, first of five, last of five."""
  _, seqs, labels, _, _ = _batch('trained_d256')
  mine, mine_labels = seqs[1], labels[1]  # the 18-cluster one
  others = [(seqs[u], labels[u]) for u in (0, 2, 3, 4)]
  dec = _capi.Decoder(_params('trained_d256'), 0)
  try:
    def run(members, at):
      frames, offsets = oracle.pack([m[0] for m in members])
      scores, rows = dec.score_speakers(frames, offsets, _cat([m[1] for m in members]), 19)
      return scores[at], rows[offsets[at]:offsets[at + 1]]
    alone = run([(mine, mine_labels)], 0)
    first = run([(mine, mine_labels)] + others, 0)
    last = run(others + [(mine, mine_labels)], 4)
  finally:
    dec.close()
  for other in (first, last):
    assert _bits(other[0]) == _bits(alone[0]) and np.array_equal(_bits(other[1]), _bits(alone[1]))


@pytest.mark.parametrize('model', ['toy_d2_depth2', 'trained_d256'])
def test_poisoned_workspace(model, monkeypatch):
  """No row depends on stale memory: the reference's bits under every poison word, the invalid trace included, on a
  handle whose buffers an earlier, larger call has already grown."""
  monkeypatch.delenv(KNOB, raising=False)
  dec = _capi.Decoder(_params(model), 0)
  try:
    _check_batch(dec, model, 'unpoisoned')
    for word in WORDS:
      monkeypatch.setenv(KNOB, word)
      _check_batch(dec, model, 'under ' + word)
  finally:
    dec.close()


def test_what_the_call_leaves_behind():
  """After score_speakers, uis_score_labels and a session prime on the same handle give a fresh handle's bits."""
  params = _params('trained_d256')
  seqs, labels = _truth_batch(3, 50, 9500)
  frames, offsets = oracle.pack(seqs)
  flat = _cat(labels)
  _, bseqs, blabels, _, _ = _batch('trained_d256')
  bframes, boffsets = oracle.pack(bseqs)

  def after(dec):
    scored = dec.score_labels(frames, offsets, flat, want_frame_losses=True)
    dec.stream_begin(3, 4, 80)
    try:
      primed = dec.stream_prime([s[:30] for s in seqs], [l[:30] for l in labels])
      dec.stream_push([s[30:] for s in seqs])
      per_utt, scores, _, _ = dec.stream_labels()
    finally:
      dec.stream_end()
    return scored, primed, per_utt, scores

  fresh, used = _capi.Decoder(params, 0), _capi.Decoder(params, 0)
  try:
    used.score_speakers(bframes, boffsets, _cat(blabels), 19)
    a, b = after(fresh), after(used)
  finally:
    fresh.close()
    used.close()
  assert np.array_equal(_bits(a[0][0]), _bits(b[0][0])) and np.array_equal(_bits(a[0][1]), _bits(b[0][1]))
  assert np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(_bits(a[3]), _bits(b[3]))
  assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))


def test_uisrnn_score_speakers():
  """The public call: ids of any kind, one [N, K + 1] array per sequence sliced from the batch's width, a single
  array for a single sequence, and speaker_posteriors on its rows."""
  argv = ['--observation_dim', '256', '--rnn_hidden_size', '512']
  model_args, _, _ = uisrnn_amd.parse_arguments(argv)
  model = uisrnn_amd.UISRNN(model_args)
  model.load(os.path.join(golden_util.GOLDEN_DIR, 'trained_d256.uisrnn'))
  _, seqs, labels, _, want_rows = _batch('trained_d256')
  pick = [1, 2, 5, 6]  # 18 clusters, one cluster, empty, one frame: widths 19, 2, 1, 2
  got = model.score_speakers([seqs[u] for u in pick], [['spk{}'.format(c) for c in labels[u]] for u in pick])
  assert isinstance(got, list) and [g.shape for g in got] == [(44, 19), (30, 2), (0, 1), (1, 2)]
  for g, u in zip(got, pick):
    assert g.dtype == np.float32 and np.array_equal(_bits(g), _bits(want_rows[u]))
  single = model.score_speakers(seqs[2], (labels[2] + 7).tolist())
  assert isinstance(single, np.ndarray) and np.array_equal(_bits(single), _bits(want_rows[2]))
  _, per = model.score_labels(seqs[1], labels[1].tolist(), per_frame=True)
  assert np.array_equal(_bits(got[0][np.arange(44), labels[1]]), _bits(per))
  post = uisrnn_amd.speaker_posteriors(got[0])
  assert post.shape == (44, 19) and np.allclose(post.sum(axis=1), 1.0) and np.all(post[np.isposinf(got[0])] == 0.0)
  assert model.last_stats is None
