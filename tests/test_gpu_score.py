"""uis_score_labels / UISRNN.score_labels on the GPU.

1. decode consistency: the labels of a test_iteration 1 decode score the decode's best score, bit for bit;
2. the CPU restatement (tests/forced_ref.py), bit for bit, totals and every per-frame loss;
3. the reference's own NLLs (tests/golden/fn_forced_scores.npz), within 1e-4 relative;
4. behaviour (renaming, invalid labels, sessions, the last decode's state, quirk 7);
5. scale.
"""

import os

import numpy as np
import pytest

import forced_ref
import golden_util
import uisrnn_amd
from oracle import oracle
from uisrnn_amd import _capi, synth, weights

pytestmark = pytest.mark.gpu


def _bits(a):
  return np.asarray(a, dtype=np.float32).view(np.uint32)


def _trained(name):
  return weights.load_checkpoint(os.path.join(golden_util.GOLDEN_DIR, name))


def _decode_then_score(params, seqs, beam, look_ahead):
  dec = _capi.Decoder(params, 0)
  frames, offsets = oracle.pack(seqs)
  out = dec.decode(frames, offsets, beam, look_ahead, 1)
  assert out['status'] == 0
  scores, losses = dec.score_labels(frames, offsets, out['labels'], want_frame_losses=True)
  assert np.array_equal(_bits(scores), _bits(out['scores'])), (scores, out['scores'])
  for u in range(len(seqs)):
    acc = np.float32(0.0)
    for v in losses[offsets[u]:offsets[u + 1]]:
      acc = np.float32(acc + v)
    assert _bits(acc) == _bits(scores[u])
  dec.close()


@pytest.mark.parametrize('n_utt,n_frames', [(4, 100), (2, 500)])
@pytest.mark.parametrize('beam,look_ahead', [(10, 1), (50, 2)])
def test_decode_consistency_trained_d256(n_utt, n_frames, beam, look_ahead):
  params = _trained('trained_d256.uisrnn')
  seqs, _ = synth.make_utterances(7000 + n_frames, n_utt, n_frames, 256)
  _decode_then_score(params, seqs, beam, look_ahead)


def test_decode_consistency_trained_d512():
  params = _trained('trained_d512.uisrnn')
  seqs, _ = synth.make_utterances(7100, 3, 150, 512)
  _decode_then_score(params, seqs, 10, 1)


@pytest.mark.parametrize('name', ['toy_d2_depth2', 'd20_h24_depth3'])
def test_decode_consistency_deep_models(name):
  case = golden_util.load_case(name)
  _decode_then_score(case['params'], case['seqs'], 4, 1)
  _decode_then_score(case['params'], case['seqs'], 3, 2)


@pytest.mark.parametrize('dim,hidden,depth', [(64, 300, 1), (180, 200, 1), (64, 320, 1), (300, 640, 1), (48, 320, 2)])
def test_decode_consistency_padded_shapes(dim, hidden, depth):
  """Padded D / H, the hidden 257..384 embedding, H > 512 and D 257..384 (a launch per step in the decode)."""
  params = synth.tracker_params(dim, hidden, depth, seed=dim + hidden)
  seqs, _ = synth.make_utterances(7200 + dim, 3, [60, 35, 80], dim)
  _decode_then_score(params, seqs, 8, 1)


def _labelings(rng, seqs):
  out = {}
  out['random'] = [forced_ref.first_appearance(rng.integers(0, 4, size=s.shape[0]).tolist()) for s in seqs]
  out['alternating'] = [np.arange(s.shape[0], dtype=np.int32) % 2 for s in seqs]
  return out


def _check_against_restatement(params, seqs, labels):
  dec = _capi.Decoder(params, 0)
  frames, offsets = oracle.pack(seqs)
  got, losses = dec.score_labels(frames, offsets, np.concatenate(labels).astype(np.int32) if seqs else
                                 np.zeros(0, np.int32), want_frame_losses=True)
  ref, ref_losses = forced_ref.score(params, seqs, labels)
  assert np.array_equal(_bits(got), _bits(ref)), (got, ref)
  assert np.array_equal(_bits(losses), _bits(np.concatenate(ref_losses)))
  for u in range(len(seqs)):
    acc = np.float32(0.0)
    for v in losses[offsets[u]:offsets[u + 1]]:
      acc = np.float32(acc + v)
    assert _bits(acc) == _bits(got[u])
  dec.close()
  return got


def test_against_restatement_labelings():
  params = synth.tracker_params(32, 48, 2, seed=5)
  seqs, truth = synth.make_utterances(7300, 3, 120, 32)
  rng = np.random.default_rng(0)
  _check_against_restatement(params, seqs, [forced_ref.first_appearance(t.tolist()) for t in truth])
  for labels in _labelings(rng, seqs).values():
    _check_against_restatement(params, seqs, labels)


def test_against_restatement_one_long_cluster_and_all_new():
  params = synth.tracker_params(32, 48, 1, seed=6)
  long_seq, _ = synth.make_utterance(7400, 1000, 32)
  _check_against_restatement(params, [long_seq], [np.zeros(1000, np.int32)])
  short, _ = synth.make_utterance(7401, 300, 32)
  _check_against_restatement(params, [short], [np.arange(300, dtype=np.int32)])  # 300 chains of length 1


def test_against_restatement_ragged_lengths():
  params = synth.tracker_params(24, 40, 1, seed=8)
  rng = np.random.default_rng(1)
  seqs = [synth.make_utterance(7500 + i, n, 24)[0] for i, n in enumerate([0, 1, 37, 0, 5, 64, 1])]
  labels = [forced_ref.first_appearance(rng.integers(0, 3, size=s.shape[0]).tolist()) for s in seqs]
  got = _check_against_restatement(params, seqs, labels)
  assert got[0] == 0.0 and got[3] == 0.0


def test_reference_fixtures():
  """The reference's neg_likelihood of truth and perturbed labelings (make_forced.py), 1e-4 relative."""
  path = os.path.join(golden_util.GOLDEN_DIR, 'fn_forced_scores.npz')
  data = np.load(path)
  worst = 0.0
  for case in [str(c) for c in data['cases']]:
    ckpt = str(data[case + '/checkpoint'])
    params = (_trained(ckpt) if ckpt.endswith('.uisrnn') else golden_util.load_case(ckpt)['params'])
    dim = int(params['observation_dim'])
    lens = data[case + '/lengths']
    seqs = [synth.make_utterance(int(data[case + '/utt_seed']) + u, int(n), dim)[0] for u, n in enumerate(lens)]
    dec = _capi.Decoder(params, 0)
    frames, offsets = oracle.pack(seqs)
    for k in range(int(data[case + '/n_labelings'])):
      labels = data['{}/labels_{}'.format(case, k)]
      ref = data['{}/scores_{}'.format(case, k)]
      got = dec.score_labels(frames, offsets, labels)
      rel = np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1e-30)
      worst = max(worst, float(rel.max()))
      assert np.all(rel <= 1e-4), (case, k, got, ref)
    dec.close()
  print('max relative difference to the reference: {:.3g}'.format(worst))


def _uisrnn_d256():
  argv = ['--observation_dim', '256', '--rnn_hidden_size', '512']
  model_args, _, inference_args = uisrnn_amd.parse_arguments(argv)
  model = uisrnn_amd.UISRNN(model_args)
  model.load(os.path.join(golden_util.GOLDEN_DIR, 'trained_d256.uisrnn'))
  return model, inference_args


def test_renamed_ids_give_identical_bits():
  model, _ = _uisrnn_d256()
  seqs, truth = synth.make_utterances(7600, 2, 90, 256)
  a = model.score_labels(seqs, [t.tolist() for t in truth])
  b = model.score_labels(seqs, [[('spk', 'wxyz'[int(v)]) for v in t] for t in truth])
  c = model.score_labels(seqs, [(np.asarray(t) * 7 + 100).tolist() for t in truth])
  d, per = model.score_labels(seqs[0], np.array(['s{}'.format(v) for v in truth[0]]), per_frame=True)
  assert isinstance(a, list) and isinstance(d, float)
  assert _bits(a).tolist() == _bits(b).tolist() == _bits(c).tolist()
  assert _bits(d) == _bits(a[0]) and per.dtype == np.float32 and per.shape == (90,)
  assert model.last_stats is None  # scoring does not touch the decode's statistics


def test_invalid_and_negative_labels_at_the_c_abi():
  params = _trained('trained_d256.uisrnn')
  seqs, _ = synth.make_utterances(7700, 2, 40, 256)
  dec = _capi.Decoder(params, 0)
  frames, offsets = oracle.pack(seqs)
  labels = np.zeros(80, dtype=np.int32)
  labels[10] = 2  # past K + 1: the reference's invalid trace
  scores, losses = dec.score_labels(frames, offsets, labels, want_frame_losses=True)
  assert np.isposinf(scores[0]) and np.isfinite(scores[1])
  assert np.all(np.isposinf(losses[10:40])) and np.all(np.isfinite(losses[:10]))
  labels[10] = -1
  with pytest.raises(_capi.HipLibraryError) as err:
    dec.score_labels(frames, offsets, labels)
  assert err.value.status == _capi.UIS_ERR_INVALID_ARG
  dec.close()


def test_refused_while_a_session_is_open():
  params = _trained('trained_d256.uisrnn')
  dec = _capi.Decoder(params, 0)
  seqs, _ = synth.make_utterances(7800, 1, 20, 256)
  frames, offsets = oracle.pack(seqs)
  dec.stream_begin(1, 4, 100)
  try:
    with pytest.raises(_capi.HipLibraryError, match='streaming session is open'):
      dec.score_labels(frames, offsets, np.zeros(20, np.int32))
  finally:
    dec.stream_end()
  assert np.isfinite(dec.score_labels(frames, offsets, np.zeros(20, np.int32))[0])
  dec.close()


def test_last_decode_state_is_left_alone():
  params = _trained('trained_d256.uisrnn')
  seqs, truth = synth.make_utterances(7900, 3, 80, 256)
  frames, offsets = oracle.pack(seqs)
  truth_cat = np.concatenate([forced_ref.first_appearance(t.tolist()) for t in truth]).astype(np.int32)

  def state(dec, score_between):
    out = dec.decode(frames, offsets, 6, 1, 2, want_beam_scores=True)
    if score_between:
      dec.score_labels(frames, offsets, truth_cat[::-1].copy() * 0, want_frame_losses=True)
    lib = dec._lib  # pylint: disable=protected-access
    n_utt, beam = np.zeros(1, np.int32), np.zeros(1, np.int32)
    lib.uis_last_decode_shape(dec._handle, n_utt.ctypes.data_as(_capi.ctypes.POINTER(_capi.ctypes.c_int32)),  # pylint: disable=protected-access
                              beam.ctypes.data_as(_capi.ctypes.POINTER(_capi.ctypes.c_int32)))
    overflow = np.zeros(3, np.int32)
    beam_scores = np.zeros((3, 6), np.float32)
    lib.uis_last_decode_info(dec._handle, overflow.ctypes.data_as(_capi.ctypes.POINTER(_capi.ctypes.c_int32)),  # pylint: disable=protected-access
                             beam_scores.ctypes.data_as(_capi._fp))  # pylint: disable=protected-access
    matched = dec.eval_last_decode(truth_cat, 3)
    return out['labels'], int(n_utt[0]), int(beam[0]), overflow, beam_scores, matched

  dec_a = _capi.Decoder(params, 0)
  dec_b = _capi.Decoder(params, 0)
  a, b = state(dec_a, False), state(dec_b, True)
  assert np.array_equal(a[0], b[0]) and a[1:3] == b[1:3] == (3, 6)
  assert np.array_equal(a[3], b[3]) and np.array_equal(_bits(a[4]), _bits(b[4])) and np.array_equal(a[5], b[5])
  dec_a.close()
  dec_b.close()


def test_quirk7_frame_matches_the_restatement():
  """A frame whose first feature equals the mean it is scored against: (a - b)^2 = 0 in dim 0 makes
  the weighted MSE +inf; the utterance goes +inf, the other one is unaffected."""
  params = synth.tracker_params(32, 48, 1, seed=9)
  seqs, _ = synth.make_utterances(8000, 2, 30, 32)
  m0, _ = oracle.constants(params)
  seqs[0] = seqs[0].copy()
  seqs[0][12, 0] = float(m0[0])  # frame 12 opens a new cluster below: scored against m0
  labels = [np.array([0] * 12 + [1] * 18, np.int32), np.array([0] * 15 + [1] * 15, np.int32)]
  got = _check_against_restatement(params, seqs, labels)
  assert np.isposinf(got[0]) and np.isfinite(got[1])


def test_scale_1024_utterances():
  params = _trained('trained_d256.uisrnn')
  seqs, truth = synth.make_utterances(8100, 1024, 1000, 256)
  dec = _capi.Decoder(params, 0)
  frames, offsets = oracle.pack(seqs)
  labels = np.concatenate([forced_ref.first_appearance(t.tolist()) for t in truth]).astype(np.int32)
  scores = dec.score_labels(frames, offsets, labels)
  assert scores.shape == (1024,) and np.all(np.isfinite(scores))
  # 8 of them: decoded with test_iteration 1, their labels score the decode's score
  pick = list(range(0, 1024, 128))
  sub = [seqs[u] for u in pick]
  f8, o8 = oracle.pack(sub)
  out = dec.decode(f8, o8, 10, 1, 1)
  assert np.array_equal(_bits(dec.score_labels(f8, o8, out['labels'])), _bits(out['scores']))
  # and scoring the truth of those 8 alone gives the same bits as inside the large call
  l8 = np.concatenate([labels[offsets[u]:offsets[u + 1]] for u in pick])
  assert np.array_equal(_bits(dec.score_labels(f8, o8, l8)), _bits(scores[pick]))
  dec.close()
