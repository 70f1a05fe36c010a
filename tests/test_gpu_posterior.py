"""Posterior readout on the GPU: uis_last_decode_posterior / uis_stream_posterior and what is built on them.

The reference is tests/posterior_ref.py (float64) fed with the rows and scores of tests/nbest_ref.py's replay of the
oracle, which the device's n-best readout equals bit for bit (tests/test_gpu_nbest.py).  Tolerance, derived in
posterior_ref.tolerance: |device - reference| <= (live + 8) * 2^-23 for confidence, change and the weights.

Every parity test first asserts ON THE REFERENCE ALONE that some utterance of its case has a frame with confidence
in (0.001, 0.999) and a frame with change in (0.001, 0.999): a kernel that returned [lab == lab_0] unweighted would
fail there.  (A beam of 1 cannot meet that condition; its results are exact instead and are checked as such.)  The
D = 256 models are so peaked that they need temperature 16 for it.  Each parity test prints its worst error
(pytest -s).
"""

import ctypes

import numpy as np
import pytest

import nbest_ref
import posterior_ref
import test_gpu_nbest as gn
import uisrnn_amd
from uisrnn_amd import _capi

pytestmark = pytest.mark.gpu

_i32p = ctypes.POINTER(ctypes.c_int32)
_ONE = np.float32(1.0).view(np.uint32)


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _refs(tag, params, seqs, beam, look=1, tau=1):
  """Per utterance (rows, scores) of the replay shared with tests/test_gpu_nbest.py; no frames: no hypothesis."""
  return [nbest_ref.nbest(gn._replay((tag, u), params, s, beam, look, tau)) if len(s) else   # pylint: disable=protected-access
          (np.zeros((0, 0), dtype=np.int32), np.zeros(0, dtype=np.float32)) for u, s in enumerate(seqs)]


def _interior(refs, temperature):
  """The condition on every parity case, from the reference alone."""
  for rows, scores in refs:
    conf, change, _ = posterior_ref.posterior(rows, scores, temperature)
    if posterior_ref.interior(conf) and posterior_ref.interior(change):
      return True
  return False


def _check(got, refs, temperature, what):
  """got = Decoder.last_posterior / stream_posterior.  Returns the worst error in units of the tolerance."""
  worst, worst_abs = 0.0, 0.0
  beam = got['weights'].shape[1]
  for u, (rows, scores) in enumerate(refs):
    live = rows.shape[0]
    conf, change, w = posterior_ref.posterior(rows, scores, temperature)
    tol = posterior_ref.tolerance(live)
    assert got['counts'][u] == live, (what, u, got['counts'][u], live)
    assert got['confidence'][u].shape == conf.shape and got['change'][u].shape == change.shape, (what, u)
    assert got['confidence'][u].dtype == np.float32 and got['change'][u].dtype == np.float32
    assert np.all(got['weights'][u][live:] == 0.0), (what, u)
    errs = [np.abs(got['weights'][u][:live].astype(np.float64) - w), np.abs(got['confidence'][u].astype(np.float64) - conf),
            np.abs(got['change'][u].astype(np.float64) - change)]
    err = max([float(e.max()) for e in errs if e.size] + [0.0])
    worst, worst_abs = max(worst, err / tol), max(worst_abs, err)
    if conf.size:
      assert _bits(got['change'][u][:1])[0] == 0, (what, u)          # change[0] is +0.0f, not merely small
      assert np.all(got['confidence'][u] <= 1.0) and np.all(got['change'][u] <= 1.0), (what, u)
    if live == 1:
      assert np.all(_bits(got['confidence'][u]) == _ONE), (what, u)
      assert np.array_equal(got['change'][u], change.astype(np.float32)), (what, u)
      assert _bits(got['weights'][u][:1])[0] == _ONE, (what, u)
  print('{}: worst |device - reference| = {:.3e} = {:.3f} of the tolerance (beam {})'.format(what, worst_abs, worst, beam))
  assert worst <= 1.0, (what, worst, worst_abs)
  return worst


def _parity(tag, params, seqs, beam, look, tau, temperature, **kw):
  refs = _refs(tag, params, seqs, beam, look, tau)
  if beam > 1:
    assert _interior(refs, temperature), 'the case has no frame that weighting matters for'
  dec = _capi.Decoder(params)
  out, _, offsets = gn._decode(dec, seqs, beam, look, tau, **kw)   # pylint: disable=protected-access
  assert out['status'] == 0 and not out['overflow'].any()
  got = dec.last_posterior(temperature)
  assert got['status'] == 0
  _check(got, refs, temperature, '{} beam {} look {} tau {} T {} {}'.format(tag, beam, look, tau, temperature, kw or ''))
  return dec, out, offsets, refs, got


def _same_bits(a, b):
  return (all(x.tobytes() == y.tobytes() for x, y in zip(a['confidence'], b['confidence'])) and
          all(x.tobytes() == y.tobytes() for x, y in zip(a['change'], b['change'])) and
          a['weights'].tobytes() == b['weights'].tobytes() and a['counts'].tobytes() == b['counts'].tobytes())


# ---- 1. parity with the reference

@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2'])
def test_small_models_equal_the_reference(name, oracle_lib):
  case = gn._case(name)   # pylint: disable=protected-access
  for beam, look, tau in [(10, 1, 1), (3, 1, 2)]:
    _parity(name, case['params'], case['seqs'], beam, look, tau, 1.0)


@pytest.mark.parametrize('beam,look,tau', [(4, 3, 1), (5, 2, 2)])
def test_window_records_equal_the_reference(beam, look, tau, oracle_lib):
  case = gn._case('d32_lookahead3')   # pylint: disable=protected-access
  _parity('d32_lookahead3', case['params'], case['seqs'], beam, look, tau, 1.0)


@pytest.mark.parametrize('flags', [0, _capi.UIS_FLAG_STEPWISE, _capi.UIS_FLAG_OWNER_SELECT])
def test_tracker_d256_every_dispatch_path(flags, oracle_lib):
  """Temperature 16: at 1 the reference itself is 1.0 on every frame of this model."""
  case = gn._case('tracker_d256')   # pylint: disable=protected-access
  _parity('tracker_d256', case['params'], case['seqs'], 10, 1, 1, 16.0, flags=flags)


def test_embedded_hidden_size(oracle_lib):
  """test_iteration 2: the readout is the second replay's frames, change[0] = 0 although step N - 1 precedes it.
  Temperature 16, chosen by the reference (at 1 and 4 no frame of this case is interior)."""
  case = gn._case('tracker_d64_h300')   # pylint: disable=protected-access
  _parity('tracker_d64_h300', case['params'], case['seqs'], 10, 1, 2, 16.0)


# ---- 2. segment and tile edges

@pytest.mark.parametrize('name,temperature', [('tracker_d256', 16.0), ('tiny_d16', 1.0)])
@pytest.mark.parametrize('beam', [1, 3, 10, 15])
def test_segment_and_tile_edges(name, temperature, beam, oracle_lib):
  """test_gpu_nbest's edge batch: the segment length goes 1 -> 2 -> 3 -> 4 (at 128 and more every segment but the
  lowest reads `change` across its lower boundary), idle last lanes, beam_n < B on the 1- and 2-frame utterances;
  beams 10 and 15 have a second group of chains, 15 a ragged one."""
  params, base = gn._edge_batch(name)   # pylint: disable=protected-access
  rep = gn._replay((name, 'edge'), params, base, beam, 1, 1)   # pylint: disable=protected-access
  refs = [nbest_ref.nbest(rep, upto=n) for n in gn._EDGE_LENGTHS]   # pylint: disable=protected-access
  assert refs[1][0].shape[0] < beam or beam == 1
  if beam > 1:
    for n, ref in zip(gn._EDGE_LENGTHS, refs):   # pylint: disable=protected-access
      assert n < 2 or _interior([ref], temperature), n    # every prefix of two frames and more, not only one of them
  if beam >= 10:
    # a turn posterior strictly inside (0, 1) AT a segment's lowest step (200 frames: segments of 4), where the record
    # below the segment decides it.  (The reference has none there at beam 3 on either model.)
    _, change, _ = posterior_ref.posterior(refs[-1][0], refs[-1][1], temperature)
    assert posterior_ref.interior(change[np.arange(200) % 4 == 0][1:]), 'no interior change at a segment boundary'
  seqs = [base[:n] for n in gn._EDGE_LENGTHS]   # pylint: disable=protected-access
  dec = _capi.Decoder(params)
  out, _, _ = gn._decode(dec, seqs, beam, 1, 1)   # pylint: disable=protected-access
  assert out['status'] == 0 and not out['overflow'].any()
  got = dec.last_posterior(temperature)
  _check(got, refs, temperature, '{} edges beam {} T {}'.format(name, beam, temperature))
  assert got['counts'][0] == 0 and got['confidence'][0].size == 0 and np.all(got['weights'][0] == 0.0)


# ---- 3. wide beam

def test_wide_beam_through_the_window_machinery(oracle_lib):
  """beam_size 300 > 256: k_window's records, k_nbest_window's table, k_posterior_window's sums over 300 hypotheses."""
  case = gn._case('tracker_d256')   # pylint: disable=protected-access
  seqs = [case['seqs'][0][:12], case['seqs'][1][:9], case['seqs'][2][:5]]
  _, _, _, refs, got = _parity('tracker_d256_short', case['params'], seqs, 300, 1, 1, 16.0)
  assert refs[0][0].shape[0] == 300 and got['counts'].tolist() == [300, 300, 52]


# ---- 4. exact cases

@pytest.mark.parametrize('name', ['tracker_d256', 'tiny_d16'])
def test_a_beam_of_one_is_exact(name):
  case = gn._case(name)   # pylint: disable=protected-access
  dec = _capi.Decoder(case['params'])
  for tau in (1, 2):
    out, _, offsets = gn._decode(dec, case['seqs'], 1, 1, tau)   # pylint: disable=protected-access
    assert out['status'] == 0
    got = dec.last_posterior(3.0)
    for u in range(len(case['seqs'])):
      labels = out['labels'][offsets[u]:offsets[u + 1]]
      assert np.all(_bits(got['confidence'][u]) == _ONE), u
      want = np.concatenate([[0.0], (labels[1:] != labels[:-1])]).astype(np.float32)
      assert got['change'][u].tobytes() == want.tobytes(), u
      assert got['counts'][u] == 1 and _bits(got['weights'][u])[0] == _ONE


def test_an_utterance_at_the_cluster_cap_reads_zeros(oracle_lib):
  """The decode returns UIS_ERR_CLUSTER_CAP (provoked as tests/test_gpu_nbest.py does): the flagged utterances
  read zeros and count 0, their neighbours what the replay says.  With max_clusters 2 the three utterances of the
  case all reach the cap; a two-frame one (two hypotheses, [0, 0] and [0, 1]) cannot."""
  case = gn._case('tracker_d256')   # pylint: disable=protected-access
  seqs = list(case['seqs']) + [case['seqs'][0][:2]]
  refs = _refs('tracker_d256', case['params'], case['seqs'], 10)
  refs.append(nbest_ref.nbest(gn._replay(('tracker_d256', 0), case['params'], case['seqs'][0], 10, 1, 1), upto=2))   # pylint: disable=protected-access
  assert _interior(refs[3:], 16.0)
  dec = _capi.Decoder(case['params'])
  out, _, _ = gn._decode(dec, seqs, 10, 1, 1, max_clusters=2)   # pylint: disable=protected-access
  assert out['status'] == _capi.UIS_ERR_CLUSTER_CAP and out['overflow'].any() and not out['overflow'][3]
  got = dec.last_posterior(16.0)
  for u in range(len(seqs)):
    if out['overflow'][u]:
      assert got['counts'][u] == 0 and not _bits(got['confidence'][u]).any() and not _bits(got['change'][u]).any()
      assert not _bits(got['weights'][u]).any() and got['confidence'][u].size == len(seqs[u])
  keep = [u for u in range(len(seqs)) if not out['overflow'][u]]
  sub = {k: [got[k][u] for u in keep] for k in ('confidence', 'change')}
  sub.update(weights=got['weights'][keep], counts=got['counts'][keep])
  _check(sub, [refs[u] for u in keep], 16.0, 'neighbours of a capped utterance')
  # a session: the status comes with everything written
  dec.stream_begin(len(seqs), 10, 64, max_clusters=2)
  try:
    dec.stream_push(seqs)
    streamed = dec.stream_posterior(16.0)
    assert streamed['status'] == _capi.UIS_ERR_CLUSTER_CAP
    assert _same_bits(streamed, got)
  finally:
    dec.stream_end()


def test_an_empty_utterance_in_the_middle_of_a_batch(oracle_lib):
  case = gn._case('tracker_d256')   # pylint: disable=protected-access
  seqs = [case['seqs'][0], case['seqs'][1][:0], case['seqs'][2]]
  full = _refs('tracker_d256', case['params'], case['seqs'], 10)
  refs = [full[0], (np.zeros((0, 0), dtype=np.int32), np.zeros(0, dtype=np.float32)), full[2]]
  assert _interior(refs, 16.0)
  dec = _capi.Decoder(case['params'])
  out, _, _ = gn._decode(dec, seqs, 10, 1, 1)   # pylint: disable=protected-access
  assert out['status'] == 0
  got = dec.last_posterior(16.0)
  _check(got, refs, 16.0, 'an empty utterance between two others')
  assert got['counts'][1] == 0 and not got['weights'][1].any()


# ---- 5. sessions

def _prefix_refs(reps, have):
  return [nbest_ref.nbest(r, upto=n) for r, n in zip(reps, have)]


@pytest.mark.parametrize('chunk', [7, 17])
def test_streaming_equals_the_offline_readout_after_every_push(chunk, oracle_lib):
  """Ragged pushes (lengths 40 / 60 / 25): after each, bit for bit the offline readout of the same prefixes on a
  second handle, and the reference at `upto`."""
  case = gn._case('tracker_d256')   # pylint: disable=protected-access
  params, seqs, beam, temperature = case['params'], case['seqs'], 10, 16.0
  reps = [gn._replay(('tracker_d256', u), params, s, beam, 1, 1) for u, s in enumerate(seqs)]   # pylint: disable=protected-access
  longest = max(len(s) for s in seqs)
  steps = [[min(len(s), lo + chunk) for s in seqs] for lo in range(0, longest, chunk)]
  assert all(_interior(_prefix_refs(reps, have), temperature) for have in steps)
  dec, offline = _capi.Decoder(params), _capi.Decoder(params)
  dec.stream_begin(len(seqs), beam, longest)
  try:
    empty = dec.stream_posterior(temperature)
    assert empty['counts'].tolist() == [0, 0, 0] and not empty['weights'].any() and empty['status'] == 0
    for lo, have in zip(range(0, longest, chunk), steps):
      dec.stream_push([s[lo:lo + chunk] if lo < len(s) else None for s in seqs])
      got = dec.stream_posterior(temperature)
      assert got['status'] == 0
      _check(got, _prefix_refs(reps, have), temperature, 'session chunk {} after {}'.format(chunk, have))
      out, _, _ = gn._decode(offline, [s[:n] for s, n in zip(seqs, have)], beam, 1, 1)   # pylint: disable=protected-access
      assert out['status'] == 0
      assert _same_bits(got, offline.last_posterior(temperature)), have
  finally:
    dec.stream_end()


def _session_ref(dec, beam):
  """The reference's inputs from the session's own n-best readout (the window's rows and scores)."""
  hyps = dec.stream_nbest(beam)
  return [(hyps['labels'][u][:int(hyps['counts'][u])], hyps['scores'][u][:int(hyps['counts'][u])])
          for u in range(len(hyps['labels']))], hyps


def test_after_a_commit_the_readout_covers_the_window(oracle_lib):
  """24 frames, commit with horizon 8 (16 leave the window, hypotheses are pruned), 6 more frames: the readout is the
  14-frame window's, equal to the reference fed with the session's own nbest() rows and scores, and change is 0 at
  the window's first frame although committed frames precede it.  (On the CPU, tests/commit_ref.py: every utterance
  of this case then has interior confidence and change at temperature 16.)  Then horizon 0 empties the windows."""
  case = gn._case('tracker_d256')   # pylint: disable=protected-access
  params, seqs, beam, temperature = case['params'], [s[:30] for s in case['seqs'][:2]] + [case['seqs'][2][:24]], 10, 16.0
  dec = _capi.Decoder(params)
  dec.stream_begin(3, beam, 32)
  try:
    dec.stream_push([s[:24] for s in seqs])
    committed, dropped = dec.stream_commit([8, 8, 8])
    assert [len(c) for c in committed] == [16, 16, 16] and dropped.sum() > 0
    dec.stream_push([seqs[0][24:], seqs[1][24:], None])
    refs, hyps = _session_ref(dec, beam)
    assert [r[0].shape[1] for r in refs] == [14, 14, 8]
    assert _interior(refs, temperature)
    got = dec.stream_posterior(temperature)
    _check(got, refs, temperature, 'the window after a commit with a horizon')
    assert all(_bits(c[:1])[0] == 0 for c in got['change'])
    again = dec.stream_nbest(beam)                        # the n-best readout finds everything as it left it
    assert all(np.array_equal(a, b) for a, b in zip(again['labels'], hyps['labels']))
    assert again['scores'].tobytes() == hyps['scores'].tobytes() and again['stable'].tolist() == hyps['stable'].tolist()
    # horizon 0 on an even window: everything is committed, one hypothesis lives, no frames are left to show
    dec.stream_commit([0, 0, -1])
    got = dec.stream_posterior(temperature)
    assert got['counts'][:2].tolist() == [1, 1] and got['confidence'][0].size == 0 and got['change'][1].size == 0
    assert np.all(_bits(got['weights'][:2, 0]) == _ONE) and not got['weights'][:2, 1:].any()
    untouched = _session_ref(dec, beam)[0][2]
    _check({k: got[k][2:] for k in ('confidence', 'change', 'weights', 'counts')}, [untouched], temperature,
           'the neighbour of two emptied windows')
  finally:
    dec.stream_end()


def test_a_restarted_slot_reads_zeros_and_the_others_keep_their_bits(oracle_lib):
  case = gn._case('tracker_d256')   # pylint: disable=protected-access
  seqs = [s[:20] for s in case['seqs']]
  dec = _capi.Decoder(case['params'])
  dec.stream_begin(3, 10, 32)
  try:
    dec.stream_push(seqs)
    before = dec.stream_posterior(16.0)
    assert before['counts'].tolist() == [10, 10, 10]
    dec.stream_restart([0, 1, 0])
    after = dec.stream_posterior(16.0)
    assert after['counts'].tolist() == [10, 0, 10] and after['confidence'][1].size == 0 and not after['weights'][1].any()
    for u in (0, 2):
      assert after['confidence'][u].tobytes() == before['confidence'][u].tobytes()
      assert after['change'][u].tobytes() == before['change'][u].tobytes()
      assert after['weights'][u].tobytes() == before['weights'][u].tobytes()
    dec.stream_push([None, seqs[1][:5], None])             # the slot is new
    assert dec.stream_posterior(16.0)['confidence'][1].size == 5
  finally:
    dec.stream_end()


def _model(params, beam):
  model_args, _, inference_args = uisrnn_amd.parse_arguments([])
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params)
  inference_args.beam_size, inference_args.look_ahead, inference_args.test_iteration = beam, 1, 1
  return model, inference_args


def test_a_persistent_session_returns_the_bits_of_an_ordinary_one_and_goes_on_decoding(oracle_lib):
  """Through OnlineSession / StreamPool / predict_posteriors.  (Where the device does not take the persistent launch
  the session runs ordinary launches and the comparison still holds.)"""
  case = gn._case('tracker_d256')   # pylint: disable=protected-access
  seqs = [np.asarray(s, dtype=np.float64) for s in case['seqs']]
  model, args = _model(case['params'], 10)
  offline = model.predict(seqs, args)
  triples = model.predict_posteriors(seqs, args, temperature=16)
  assert [t[0] for t in triples] == offline
  one = model.predict_posteriors(seqs[1], args, temperature=16)
  assert one[0] == offline[1] and one[1].tobytes() == triples[1][1].tobytes() and one[2].tobytes() == triples[1][2].tobytes()
  refs = _refs('tracker_d256', case['params'], case['seqs'], 10)
  for u, (rows, scores) in enumerate(refs):
    conf, change, _ = posterior_ref.posterior(rows, scores, 16.0)
    assert np.abs(triples[u][1] - conf).max() <= posterior_ref.tolerance(rows.shape[0])
    assert np.abs(triples[u][2] - change).max() <= posterior_ref.tolerance(rows.shape[0])
  got = {}
  for persistent in (False, True):
    with model.online_pool(3, args, max_frames=64, persistent=persistent) as pool:
      for u in range(3):
        pool.open(u)
      pool.push({u: s[:17] for u, s in enumerate(seqs)})
      got[persistent] = [pool.posteriors(u, temperature=16) for u in range(3)]
      pool.push({u: s[17:] for u, s in enumerate(seqs)})                  # the next push still decodes
      assert [pool.labels(u) for u in range(3)] == offline
      final = pool._session.posteriors(16)   # pylint: disable=protected-access
      for u in range(3):
        assert final[u][0].tobytes() == triples[u][1].tobytes() and final[u][1].tobytes() == triples[u][2].tobytes()
        assert len(final[u][2]) == refs[u][0].shape[0]
  for a, b in zip(got[False], got[True]):
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
  with pytest.raises(ValueError, match='temperature'):
    model.predict_posteriors(seqs, args, temperature=0)


# ---- 6. the call leaves everything alone

def _raw(dec, fn, temperature, total, n_utt, beam, capacity=None):
  conf = np.full(total + 8, -7, dtype=np.float32)
  change = np.full(total + 8, -7, dtype=np.float32)
  weights = np.full(n_utt * beam + 8, -7, dtype=np.float32)
  counts = np.full(n_utt + 8, -7, dtype=np.int32)
  rc = fn(dec._handle, temperature, conf.ctypes.data_as(_capi._fp), change.ctypes.data_as(_capi._fp),   # pylint: disable=protected-access
          total if capacity is None else capacity, weights.ctypes.data_as(_capi._fp), counts.ctypes.data_as(_i32p))
  return rc, conf, change, weights, counts


def test_the_call_leaves_everything_alone_and_its_state_rules():
  case = gn._case('tracker_d256')   # pylint: disable=protected-access
  seqs = case['seqs']
  total = sum(len(s) for s in seqs)
  dec = _capi.Decoder(case['params'])
  last, stream = dec._lib.uis_last_decode_posterior, dec._lib.uis_stream_posterior   # pylint: disable=protected-access
  assert _raw(dec, last, 16.0, total, 3, 10)[0] == _capi.UIS_ERR_INVALID_ARG            # no decode yet
  assert _raw(dec, stream, 16.0, total, 3, 10)[0] == _capi.UIS_ERR_INVALID_ARG          # no session
  out, frames, offsets = gn._decode(dec, seqs, 10, 1, 2)   # pylint: disable=protected-access
  assert out['status'] == 0
  info = np.empty((3, 10), dtype=np.float32)
  over = np.empty(3, dtype=np.int32)
  assert dec._lib.uis_last_decode_info(dec._handle, over.ctypes.data_as(_i32p), info.ctypes.data_as(_capi._fp)) == 0   # pylint: disable=protected-access
  truth = np.concatenate([np.arange(len(s)) % 3 for s in seqs]).astype(np.int32)
  matched = dec.eval_last_decode(truth, 3).copy()
  hyps = dec.last_nbest(10)

  first = _raw(dec, last, 16.0, total, 3, 10)
  assert first[0] == 0
  assert np.all(first[1][total:] == -7) and np.all(first[2][total:] == -7) and np.all(first[3][30:] == -7) and np.all(first[4][3:] == -7)
  for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float('nan')), dict(temperature=float('inf')),
              dict(capacity=total - 1)):
    refused = _raw(dec, last, bad.get('temperature', 16.0), total, 3, 10, bad.get('capacity'))
    assert refused[0] == _capi.UIS_ERR_INVALID_ARG, bad
    assert all(np.all(a == -7) for a in refused[1:]), bad                           # ... and touches nothing
  second = _raw(dec, last, 16.0, total, 3, 10)                                      # two calls: identical bits
  assert second[0] == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(first[1:], second[1:]))
  other = _raw(dec, last, 4.0, total, 3, 10)                                        # the temperature is not decoration
  assert other[0] == 0 and other[3].tobytes() != first[3].tobytes()
  # NULL outputs are fine
  assert last(dec._handle, 16.0, None, None, 0, None, None) == 0   # pylint: disable=protected-access
  only = np.full(total, -7, dtype=np.float32)
  assert last(dec._handle, 16.0, None, only.ctypes.data_as(_capi._fp), total, None, None) == 0   # pylint: disable=protected-access
  assert only.tobytes() == first[2][:total].tobytes()

  again = dec.last_nbest(10)
  assert all(np.array_equal(a, b) for a, b in zip(again['labels'], hyps['labels']))
  assert again['scores'].tobytes() == hyps['scores'].tobytes() and again['counts'].tobytes() == hyps['counts'].tobytes()
  info2 = np.empty((3, 10), dtype=np.float32)
  over2 = np.empty(3, dtype=np.int32)
  assert dec._lib.uis_last_decode_info(dec._handle, over2.ctypes.data_as(_i32p), info2.ctypes.data_as(_capi._fp)) == 0   # pylint: disable=protected-access
  assert info2.tobytes() == info.tobytes() and over2.tobytes() == over.tobytes()
  assert np.array_equal(dec.eval_last_decode(truth, 3), matched)
  n_utt, beam = ctypes.c_int32(0), ctypes.c_int32(0)
  assert dec._lib.uis_last_decode_shape(dec._handle, ctypes.byref(n_utt), ctypes.byref(beam)) == 0   # pylint: disable=protected-access
  assert (n_utt.value, beam.value) == (3, 10)

  dec.stream_begin(2, 4, 8)                                                         # an open session
  assert _raw(dec, last, 16.0, total, 3, 10)[0] == _capi.UIS_ERR_INVALID_ARG
  dec.stream_push([seqs[0][:5], seqs[1][:3]])
  assert _raw(dec, stream, 16.0, 8, 2, 4, capacity=7)[0] == _capi.UIS_ERR_INVALID_ARG
  assert _raw(dec, stream, 0.0, 8, 2, 4)[0] == _capi.UIS_ERR_INVALID_ARG
  assert _raw(dec, stream, 16.0, 8, 2, 4)[0] == 0
  dec.stream_end()
  third = _raw(dec, last, 16.0, total, 3, 10)                                       # ... and the decode's state is intact
  assert third[0] == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(first[1:], third[1:]))
  redo, _, _ = gn._decode(dec, seqs, 10, 1, 2)   # pylint: disable=protected-access
  assert np.array_equal(redo['labels'], out['labels'])                              # a decode after the call: the same labels

  # two utterance groups, each read from its own saved state
  gn._decode(dec, seqs, 10, 1, 2, flags=_capi.UIS_FLAG_STEPWISE, n_streams=2)   # pylint: disable=protected-access
  grouped = _raw(dec, last, 16.0, total, 3, 10)
  assert grouped[0] == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(first[1:], grouped[1:]))


# ---- 7. stale memory

@pytest.mark.parametrize('name,beam,look,temperature', [('tracker_d256', 10, 1, 16.0), ('tiny_d16', 3, 1, 1.0),
                                                        ('d32_lookahead3', 4, 3, 1.0)])
def test_no_result_depends_on_stale_memory(name, beam, look, temperature, oracle_lib, monkeypatch):
  """UIS_POISON_WORKSPACE (uisrnn_amd/csrc/uis_poison.h) under two words: the readout's own buffers are filled before
  it runs, the decode's workspace before the decode; the bits are those of the unpoisoned run."""
  case = gn._case(name)   # pylint: disable=protected-access
  refs = _refs(name, case['params'], case['seqs'], beam, look, 1)
  assert _interior(refs, temperature)
  monkeypatch.delenv('UIS_POISON_WORKSPACE', raising=False)
  dec = _capi.Decoder(case['params'])
  try:
    gn._decode(dec, case['seqs'], beam, look, 1)   # pylint: disable=protected-access
    clean = dec.last_posterior(temperature)
    _check(clean, refs, temperature, '{} unpoisoned'.format(name))
    for word in ('ffffffff', '7f7f7f7f'):
      monkeypatch.setenv('UIS_POISON_WORKSPACE', word)
      assert _same_bits(dec.last_posterior(temperature), clean), word             # the readout alone
      out, _, _ = gn._decode(dec, case['seqs'], beam, look, 1)   # pylint: disable=protected-access
      assert out['status'] == 0
      assert _same_bits(dec.last_posterior(temperature), clean), word             # ... and after a poisoned decode
    if look == 1:
      dec.stream_begin(len(case['seqs']), beam, max(len(s) for s in case['seqs']))
      try:
        dec.stream_push(list(case['seqs']))
        assert _same_bits(dec.stream_posterior(temperature), clean)
      finally:
        dec.stream_end()
  finally:
    dec.close()
