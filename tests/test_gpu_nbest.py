"""N-best readout on the GPU: uis_last_decode_nbest / uis_stream_nbest and what is built on them.

The reference for every rank's labels is tests/nbest_ref.py: the beam history rebuilt on the CPU from
the oracle's candidate scores (checked against the oracle itself in tests/test_nbest_host.py).  All
comparisons are exact: labels are integers and the scores are the decode's own float32 words.
"""

import ctypes

import numpy as np
import pytest

import golden_util
import nbest_ref
import uisrnn_amd
from uisrnn_amd import _capi
from uisrnn_amd import synth
from uisrnn_amd import uisrnn as host

pytestmark = pytest.mark.gpu

_i32p = ctypes.POINTER(ctypes.c_int32)
_REPLAYS = {}


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _case(name):
  if name not in _REPLAYS:
    _REPLAYS[name] = golden_util.load_case(name)
  return _REPLAYS[name]


def _replay(tag, params, seq, beam, look=1, tau=1):
  """One CPU replay per (case, utterance, options), shared by every test of this file."""
  key = (tag, beam, look, tau)
  if key not in _REPLAYS:
    _REPLAYS[key] = nbest_ref.replay(params, seq, beam, look, tau)
  return _REPLAYS[key]


def _decode(dec, seqs, beam, look, tau, **kw):
  frames = (np.concatenate(seqs) if seqs else np.zeros((0, dec.observation_dim))).astype(np.float32)
  offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
  out = dec.decode(frames, offsets, beam, look, tau, want_beam_scores=True, **kw)
  return out, frames, offsets


def _compare(out, offsets, got, refs, n_best):
  """got = Decoder.last_nbest / stream_nbest; refs = per utterance (rows, scores) of the replay."""
  for u, (rows, scores) in enumerate(refs):
    live = rows.shape[0] if offsets[u + 1] > offsets[u] else 0
    cnt = min(n_best, live)
    assert got['counts'][u] == cnt, (u, got['counts'][u], cnt)
    assert np.array_equal(got['labels'][u][:cnt], rows[:cnt]), u
    assert np.all(got['labels'][u][cnt:] == -1), u
    assert np.array_equal(_bits(got['scores'][u][:cnt]), _bits(scores[:cnt])), u
    assert np.all(np.isposinf(got['scores'][u][cnt:])), u
    if out is not None:
      assert np.array_equal(_bits(got['scores'][u]), _bits(out['beam_scores'][u][:n_best])), u
      if cnt:
        assert np.array_equal(got['labels'][u][0], out['labels'][offsets[u]:offsets[u + 1]]), u


def _parity(tag, params, seqs, beam, look, tau, n_bests=None, **kw):
  dec = _capi.Decoder(params)
  refs = [nbest_ref.nbest(_replay((tag, u), params, s, beam, look, tau)) if len(s) else
          (np.zeros((0, 0), dtype=np.int32), np.zeros(0, dtype=np.float32)) for u, s in enumerate(seqs)]
  out, _, offsets = _decode(dec, seqs, beam, look, tau, **kw)
  assert out['status'] == 0 and not out['overflow'].any()
  for n_best in n_bests or (beam,):
    _compare(out, offsets, dec.last_nbest(n_best), refs, n_best)
  return dec, out, offsets, refs


# ---- 1. parity with the replay

@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2'])
def test_small_models_every_rank_equals_the_replay(name, oracle_lib):
  case = _case(name)
  for beam, look, tau in [(10, 1, 1), (10, 1, 2), (3, 1, 2)]:
    _parity(name, case['params'], case['seqs'], beam, look, tau, n_bests=(beam, 1))


@pytest.mark.parametrize('beam,look,tau', [(4, 3, 1), (5, 2, 2)])
def test_window_records_every_rank_equals_the_replay(beam, look, tau, oracle_lib):
  case = _case('d32_lookahead3')
  _parity('d32_lookahead3', case['params'], case['seqs'], beam, look, tau, n_bests=(beam, 2))


@pytest.mark.parametrize('tau', [1, 2])
@pytest.mark.parametrize('flags', [0, _capi.UIS_FLAG_STEPWISE, _capi.UIS_FLAG_OWNER_SELECT])
def test_tracker_d256_every_dispatch_path(tau, flags, oracle_lib):
  case = _case('tracker_d256')   # lengths 40 / 60 / 25; with tau 2 rows may coincide: trace[-N:] of distinct traces
  _parity('tracker_d256', case['params'], case['seqs'], 10, 1, tau, flags=flags)


def test_wide_beam_through_the_window_machinery(oracle_lib):
  """beam_size 300 > 256: look_ahead 1 decoded by k_window, its records read by k_nbest_window.  Short
  utterances: Bell(7) = 877 > 300, so the beam fills and prunes from the seventh frame on."""
  case = _case('tracker_d256')
  seqs = [case['seqs'][0][:12], case['seqs'][1][:9], case['seqs'][2][:5]]
  _parity('tracker_d256_short', case['params'], seqs, 300, 1, 1, n_bests=(300, 7))


def test_embedded_hidden_size(oracle_lib):
  case = _case('tracker_d64_h300')
  _parity('tracker_d64_h300', case['params'], case['seqs'], 10, 1, 2)


# ---- 2. segment and tile edges

_EDGE_LENGTHS = [0, 1, 2, 63, 64, 65, 128, 129, 200]


def _edge_batch(name):
  """The lengths at which k_nbest changes shape (segment length 1 -> 2 -> 3 -> 4, idle last lanes,
  beam_n < B on the 1- and 2-frame utterances), as prefixes of ONE 200-frame utterance: with
  test_iteration 1 a single replay per beam serves them all."""
  if name == 'tracker_d256':
    params = synth.tracker_params(256, 512, 1, seed=0)
    base = synth.make_utterances(13_000, 1, [200], 256)[0][0]
  else:
    case = _case(name)
    base = np.concatenate(case['seqs'] * 3)[:200]
  return params if name == 'tracker_d256' else case['params'], base


@pytest.mark.parametrize('name', ['tracker_d256', 'tiny_d16'])
@pytest.mark.parametrize('beam', [1, 3, 10, 15])
def test_segment_and_tile_edges(name, beam, oracle_lib):
  params, base = _edge_batch(name)
  rep = _replay((name, 'edge'), params, base, beam, 1, 1)
  refs = [nbest_ref.nbest(rep, upto=n) for n in _EDGE_LENGTHS]
  assert refs[1][0].shape[0] < beam or beam == 1     # beam_n < B after one frame
  seqs = [base[:n] for n in _EDGE_LENGTHS]
  dec = _capi.Decoder(params)
  out, _, offsets = _decode(dec, seqs, beam, 1, 1)
  assert out['status'] == 0 and not out['overflow'].any()
  for n_best in sorted({1, min(3, beam), beam}):
    _compare(out, offsets, dec.last_nbest(n_best), refs, n_best)


# ---- 3. consistency with score_labels

def _check_rescoring(dec, seqs, beam):
  out, frames, offsets = _decode(dec, seqs, beam, 1, 1)
  assert out['status'] == 0
  got = dec.last_nbest(beam)
  assert got['counts'].tolist() == [beam] * len(seqs)
  for k in range(beam):
    labels = np.concatenate([got['labels'][u][k] for u in range(len(seqs))])
    rescored = dec.score_labels(frames, offsets, labels)
    assert np.array_equal(_bits(rescored), _bits(got['scores'][:, k])), k
  # score_labels ran `beam` times in between: the readout is still the same
  again = dec.last_nbest(beam)
  assert all(np.array_equal(a, b) for a, b in zip(again['labels'], got['labels']))


def test_every_rank_rescored_by_score_labels_is_its_beam_score_tracker():
  case = _case('tracker_d256')
  _check_rescoring(_capi.Decoder(case['params']), case['seqs'], 10)


def test_every_rank_rescored_by_score_labels_is_its_beam_score_trained():
  case = golden_util.load_trained('trained_d256_n100')
  _check_rescoring(_capi.Decoder(case['params']), case['seqs'][:4], 10)


# ---- 4. exhaustive on the device

def _growth_strings(n):
  out = [[0]]
  for _ in range(1, n):
    out = [s + [c] for s in out for c in range(max(s) + 2)]
  return sorted(tuple(s) for s in out)


@pytest.mark.parametrize('n,beam', [(4, 15), (5, 52)])
def test_a_beam_of_bell_n_returns_every_partition_once(n, beam):
  """B = Bell(N): nothing is ever pruned.  15 x 17 = 255 candidates take the fast select, 52 the generic one."""
  case = _case('tracker_d256')
  dec = _capi.Decoder(case['params'])
  out, _, _ = _decode(dec, [case['seqs'][0][:n]], beam, 1, 1)
  assert out['status'] == 0
  got = dec.last_nbest(beam)
  assert got['counts'][0] == beam
  assert sorted(tuple(r) for r in got['labels'][0].tolist()) == _growth_strings(n)
  assert np.all(np.diff(got['scores'][0]) >= 0) and np.all(np.isfinite(got['scores'][0]))


# ---- 5. state rules at the C ABI

def _raw_nbest(dec, n_best, total, n_utt, capacity=None):
  labels = np.full(max(n_best, 1) * total + 8, -7, dtype=np.int32)
  scores = np.full(n_utt * max(n_best, 1), -7, dtype=np.float32)
  counts = np.full(n_utt, -7, dtype=np.int32)
  rc = dec._lib.uis_last_decode_nbest(dec._handle, n_best, labels.ctypes.data_as(_i32p),
                                      n_best * total if capacity is None else capacity,
                                      scores.ctypes.data_as(_capi._fp), counts.ctypes.data_as(_i32p))
  return rc, labels, scores, counts


def test_state_rules_at_the_c_abi():
  case = _case('tracker_d256')
  seqs = case['seqs']
  total = sum(len(s) for s in seqs)
  dec = _capi.Decoder(case['params'])
  assert _raw_nbest(dec, 3, total, 3)[0] == _capi.UIS_ERR_INVALID_ARG            # no decode yet
  out, frames, offsets = _decode(dec, seqs, 10, 1, 2)
  assert out['status'] == 0
  info_before = np.empty((3, 10), dtype=np.float32)
  over_before = np.empty(3, dtype=np.int32)
  assert dec._lib.uis_last_decode_info(dec._handle, over_before.ctypes.data_as(_i32p), info_before.ctypes.data_as(_capi._fp)) == 0
  truth = np.concatenate([np.arange(len(s)) % 3 for s in seqs]).astype(np.int32)
  matched_before = dec.eval_last_decode(truth, 3).copy()

  rc, labels, scores, counts = _raw_nbest(dec, 10, total, 3)
  assert rc == 0 and np.all(labels[10 * total:] == -7)                            # nothing past n_best * frames
  for bad in (dict(n_best=0), dict(n_best=11), dict(n_best=10, capacity=10 * total - 1)):
    assert _raw_nbest(dec, bad['n_best'], total, 3, bad.get('capacity'))[0] == _capi.UIS_ERR_INVALID_ARG, bad
  rc2, labels2, scores2, counts2 = _raw_nbest(dec, 10, total, 3)                 # the handle is still usable
  assert rc2 == 0
  assert labels2.tobytes() == labels.tobytes() and scores2.tobytes() == scores.tobytes() and counts2.tobytes() == counts.tobytes()

  dec.score_labels(frames, offsets, out['labels'])
  dec.eval_matched(truth, out['labels'], offsets)
  rc3, labels3, scores3, counts3 = _raw_nbest(dec, 10, total, 3)
  assert rc3 == 0
  assert labels3.tobytes() == labels.tobytes() and scores3.tobytes() == scores.tobytes() and counts3.tobytes() == counts.tobytes()

  info_after = np.empty((3, 10), dtype=np.float32)
  over_after = np.empty(3, dtype=np.int32)
  assert dec._lib.uis_last_decode_info(dec._handle, over_after.ctypes.data_as(_i32p), info_after.ctypes.data_as(_capi._fp)) == 0
  assert info_after.tobytes() == info_before.tobytes() and over_after.tobytes() == over_before.tobytes()
  assert np.array_equal(dec.eval_last_decode(truth, 3), matched_before)
  n_utt, beam = ctypes.c_int32(0), ctypes.c_int32(0)
  assert dec._lib.uis_last_decode_shape(dec._handle, ctypes.byref(n_utt), ctypes.byref(beam)) == 0
  assert (n_utt.value, beam.value) == (3, 10)

  # NULL scores / counts are fine
  lab = np.empty(total, dtype=np.int32)
  assert dec._lib.uis_last_decode_nbest(dec._handle, 1, lab.ctypes.data_as(_i32p), total, None, None) == 0
  assert np.array_equal(lab, out['labels'])

  dec.stream_begin(2, 4, 8)                                                       # an open session
  assert _raw_nbest(dec, 3, total, 3)[0] == _capi.UIS_ERR_INVALID_ARG
  dec.stream_end()
  assert _raw_nbest(dec, 10, total, 3)[1].tobytes() == labels.tobytes()           # ... and the decode's state is intact
  # a session that reads its labels becomes what uis_last_decode_info / _shape describe (beam 4 here): the
  # readout of the older decode goes with them, so that the three never answer for different decodes
  dec.stream_begin(2, 4, 8)
  dec.stream_push([seqs[0][:5], seqs[1][:3]])
  dec.stream_labels()
  dec.stream_end()
  assert dec._lib.uis_last_decode_shape(dec._handle, ctypes.byref(n_utt), ctypes.byref(beam)) == 0
  assert (n_utt.value, beam.value) == (2, 4)
  assert _raw_nbest(dec, 3, total, 3)[0] == _capi.UIS_ERR_INVALID_ARG
  out, frames, offsets = _decode(dec, seqs, 10, 1, 2)                             # ... until the next decode
  assert _raw_nbest(dec, 10, total, 3)[1].tobytes() == labels.tobytes()
  # a decode refused before it starts (a negative frame count) leaves nothing to read either
  lens = np.array([5, -1], dtype=np.int64)
  ptrs = (ctypes.c_void_p * 2)(None, None)
  assert dec._lib.uis_decode_f64(dec._handle, ptrs, lens.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 2,
                                 ctypes.byref(_capi.make_opts(10, 1, 1)), None, None, None) == _capi.UIS_ERR_INVALID_ARG
  assert _raw_nbest(dec, 3, total, 3)[0] == _capi.UIS_ERR_INVALID_ARG
  _decode(dec, seqs, 10, 1, 2)

  # a decode that fails otherwise leaves nothing to read
  sink = np.empty(total, dtype=np.int32)
  assert dec._lib.uis_decode(dec._handle, frames.ctypes.data_as(_capi._fp), offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 3,
                             ctypes.byref(_capi.make_opts(10, 0, 1)), sink.ctypes.data_as(_i32p), None,
                             None) == _capi.UIS_ERR_INVALID_ARG   # look_ahead 0
  assert _raw_nbest(dec, 3, total, 3)[0] == _capi.UIS_ERR_INVALID_ARG

  # two utterance groups, each read from its own saved state
  one = _decode(dec, seqs, 10, 1, 2, flags=_capi.UIS_FLAG_STEPWISE, n_streams=1)[0]
  got1 = dec.last_nbest(10)
  two = _decode(dec, seqs, 10, 1, 2, flags=_capi.UIS_FLAG_STEPWISE, n_streams=2)[0]
  assert two['stats']['n_streams'] == 2 and one['stats']['n_streams'] == 1
  got2 = dec.last_nbest(10)
  assert all(np.array_equal(a, b) for a, b in zip(got1['labels'], got2['labels']))
  assert got1['scores'].tobytes() == got2['scores'].tobytes() and got1['counts'].tobytes() == got2['counts'].tobytes()
  assert got1['scores'].tobytes() == scores.tobytes()


def test_an_utterance_at_the_cluster_cap_has_no_hypotheses():
  """UIS_ERR_CLUSTER_CAP: the flagged utterances count 0 and read -1, the others are complete."""
  case = _case('tracker_d256')
  dec = _capi.Decoder(case['params'])
  ample, _, offsets = _decode(dec, case['seqs'], 10, 1, 1)
  want = dec.last_nbest(10)
  out, _, _ = _decode(dec, case['seqs'], 10, 1, 1, max_clusters=2)
  assert out['status'] == _capi.UIS_ERR_CLUSTER_CAP and out['overflow'].any()
  got = dec.last_nbest(10)
  for u in range(3):
    if out['overflow'][u]:
      assert got['counts'][u] == 0 and np.all(got['labels'][u] == -1)
    else:
      assert got['counts'][u] == want['counts'][u] and np.array_equal(got['labels'][u], want['labels'][u])


# ---- 6. the retry path of predict_nbest

def _model(params):
  model_args, _, inference_args = uisrnn_amd.parse_arguments([])
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params)
  inference_args.beam_size, inference_args.look_ahead, inference_args.test_iteration = 10, 1, 1
  return model, inference_args


def test_predict_nbest_reads_each_utterance_after_its_own_decode():
  case = _case('tracker_d256')
  seqs = [np.asarray(s, dtype=np.float64) for s in case['seqs']] + [np.asarray(case['seqs'][0][:1], dtype=np.float64)]
  model, args = _model(case['params'])
  args.max_clusters = 16
  ample = model.predict_nbest(seqs, args)
  assert model._single_pass
  plain = model.predict(seqs, args)
  args.max_clusters = 2
  tight = model.predict_nbest(seqs, args, n_best=10)
  assert not model._single_pass                      # the cap was doubled at least once
  flagged = model._get_decoder().decode_f64(seqs, 10, 1, 1, max_clusters=2)['overflow']
  assert flagged.any() and not flagged.all()          # ... for some utterances, not for all: two different decode calls are read
  assert tight == ample
  for u, (labelings, scores) in enumerate(tight):
    assert labelings[0] == plain[u]
    assert len(labelings) == len(scores) and scores == sorted(scores)
    assert all(isinstance(x, float) for x in scores)
  assert len(tight[3][0]) == 1 and len(tight[0][0]) == 10   # one frame: one hypothesis
  # fewer than the beam, one array instead of a list
  labelings, scores = model.predict_nbest(seqs[1], args, n_best=3)
  assert labelings == ample[1][0][:3] and scores == ample[1][1][:3]
  assert model.predict(seqs, args) == plain           # predict itself is as before
  bad = seqs[2].copy()
  bad[7, 3] = np.nan
  with pytest.raises(host.EmptyBeamError):
    model.predict_nbest([seqs[0], bad], args)


# ---- 7. streaming

def _stream_case(name):
  case = _case(name)
  seqs = case['seqs'][:3] if name == 'tracker_d256' else case['seqs'][:1]
  return case['params'], seqs


def _stream_refs(name, params, seqs, beam):
  return [_replay((name, u), params, s, beam, 1, 1) for u, s in enumerate(seqs)]


def test_the_replays_stable_prefix_moves():
  """What the streaming tests below rely on: the reference's stable prefix takes several values."""
  params, seqs = _stream_case('tracker_d256')
  rep = _stream_refs('tracker_d256', params, seqs, 10)[1]
  assert sorted({nbest_ref.common_prefix(nbest_ref.nbest(rep, upto=n)[0]) for n in range(1, 61)}) == [1, 2, 7, 41]
  params, seqs = _stream_case('tiny_d16')
  rep = _stream_refs('tiny_d16', params, seqs, 3)[0]
  seen = {nbest_ref.common_prefix(nbest_ref.nbest(rep, upto=n)[0]) for n in range(1, len(seqs[0]) + 1)}
  assert sorted(seen) == [1, 8, 10, 12, 13, 21]


@pytest.mark.parametrize('name', ['tracker_d256', 'tiny_d16'])
@pytest.mark.parametrize('beam', [10, 4, 3])
@pytest.mark.parametrize('chunk', [1, 7, 16, 17])
def test_streaming_equals_the_replay_after_every_push(name, beam, chunk, oracle_lib):
  params, seqs = _stream_case(name)
  reps = _stream_refs(name, params, seqs, beam)
  finals = [nbest_ref.nbest(r)[0][0] for r in reps]
  dec = _capi.Decoder(params)
  longest = max(len(s) for s in seqs)
  dec.stream_begin(len(seqs), beam, longest)
  try:
    empty = dec.stream_nbest(beam)
    assert empty['counts'].tolist() == [0] * len(seqs) and empty['stable'].tolist() == [0] * len(seqs)
    last = np.zeros(len(seqs), dtype=np.int64)
    distinct = [set() for _ in seqs]
    for lo in range(0, longest, chunk):
      dec.stream_push([s[lo:lo + chunk] if lo < len(s) else None for s in seqs])
      have = [min(len(s), lo + chunk) for s in seqs]
      refs = [nbest_ref.nbest(r, upto=n) for r, n in zip(reps, have)]
      got = dec.stream_nbest(beam)
      assert got['status'] == 0
      _compare(None, np.concatenate([[0], np.cumsum(have)]), got, refs, beam)
      want_stable = [nbest_ref.common_prefix(rows) for rows, _ in refs]
      assert got['stable'].tolist() == want_stable, (lo, got['stable'], want_stable)
      assert np.all(got['stable'] >= last)
      last = got['stable'].copy()
      labels = dec.stream_labels()[0]
      for u in range(len(seqs)):
        assert np.array_equal(labels[u], got['labels'][u][0])
        assert np.array_equal(labels[u][:last[u]], finals[u][:last[u]]), (u, lo)
        distinct[u].add(int(last[u]))
      few = dec.stream_nbest(2 if beam > 2 else 1)     # n_best < beam_n: the stable prefix still looks at every live one
      assert few['stable'].tolist() == want_stable
    if chunk == 1 and (name, beam) in (('tracker_d256', 10), ('tiny_d16', 3)):
      assert max(len(d) for d in distinct) >= 3
  finally:
    dec.stream_end()


@pytest.mark.parametrize('beam', [10, 4, 3])
@pytest.mark.parametrize('chunk', [1, 7, 16, 17])
def test_persistent_session_nbest_and_stable_frames(beam, chunk, oracle_lib):
  """The streaming test above on a persistent session, through OnlineSession: every readout makes the
  resident launch leave and the next push start a new one (17 frames per push still fit the mailbox)."""
  params, seqs = _stream_case('tracker_d256')
  seqs = [np.asarray(s, dtype=np.float64) for s in seqs]
  reps = _stream_refs('tracker_d256', params, seqs, beam)
  model, args = _model(params)
  args.beam_size = beam
  offline = model.predict(seqs, args)
  assert [r.tolist() for r in (nbest_ref.nbest(rep)[0][0] for rep in reps)] == offline
  longest = max(len(s) for s in seqs)
  with model.online(len(seqs), args, max_frames=longest, persistent=True) as session:
    if not session.persistent:
      pytest.skip('this device does not take the persistent launch for the session')
    last = [0] * len(seqs)
    for lo in range(0, longest, chunk):
      session.push([s[lo:lo + chunk] if lo < len(s) else None for s in seqs])
      if lo + chunk >= longest:
        break                         # the last push is read below, as a session's caller would
      have = [min(len(s), lo + chunk) for s in seqs]
      refs = [nbest_ref.nbest(r, upto=n) for r, n in zip(reps, have)]
      got = session.nbest()
      for u, (rows, scores) in enumerate(refs):
        assert got[u][0] == rows.tolist(), (u, lo)
        assert np.array_equal(_bits(got[u][1]), _bits(scores)), (u, lo)
      stable = session.stable_frames()
      assert stable == [nbest_ref.common_prefix(rows) for rows, _ in refs], lo
      assert all(a >= b for a, b in zip(stable, last)), (lo, stable, last)
      last = stable
      labels = session.labels()
      assert labels == [g[0][0] for g in got]
      for u in range(len(seqs)):
        assert labels[u][:stable[u]] == offline[u][:stable[u]], (u, lo)
      assert session.persistent       # the readouts did not make the session fall back
    # the push after the launch left for a readout was taken by a new launch
    assert session.persistent
    assert session.labels() == offline
    assert [g[0][0] for g in session.nbest(1)] == offline
    assert all(a >= b for a, b in zip(session.stable_frames(), last))


def test_online_session_overflow_is_the_error_of_labels():
  case = _case('tracker_d256')
  model, args = _model(case['params'])
  args.max_clusters = 2
  with model.online(1, args, max_frames=60) as session:
    session.push([np.asarray(case['seqs'][1], dtype=np.float64)])
    with pytest.raises(RuntimeError, match='need more than max_clusters'):
      session.labels()
    with pytest.raises(RuntimeError, match='need more than max_clusters'):
      session.nbest()
    with pytest.raises(RuntimeError, match='need more than max_clusters'):
      session.stable_frames()
