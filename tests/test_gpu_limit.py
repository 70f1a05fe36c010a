"""max_speakers on the GPU against tests/limit_ref.py, bit for bit.

  1. one bounded decode per instantiation of the one-launch decode kernels (every case of tests/instantiation_cases.py
     at its own shapes, limits cycling over the utterances), the launch-per-step path and UIS_FLAG_NO_DEDUP with it;
  2. the host's regroupings through predict and the other Python entries: the float64 list in two launches, the
     overflow retry, the look-ahead level retry, the shards of parallel_predict, the n-best / posterior / primed entries;
  3. sessions: any chunking equals the offline bounded decode; limits raised and lowered mid-stream; retire, restart,
     import;
  4. a bounded session never sets the overflow word where the unbounded one does;
  5. score_labels of a bounded decode's labels, stale state on one handle (also under UIS_POISON_WORKSPACE), the cap
     policy of a wide beam.
The reference runs on the CPU: the utterances stay at the case table's lengths.
"""

import functools

import numpy as np
import pytest

import instantiation_cases as ic
import limit_ref
import posterior_ref
import primed_ref
import retire_ref
import uisrnn_amd
from oracle import oracle
from uisrnn_amd import _capi

pytestmark = pytest.mark.gpu

CYCLE = (0, 1, 2, 3)
PHASE = 1   # utterance u decodes under CYCLE[(u + PHASE) % 4]: the first one, never a single frame, under limit 1


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _n_cu():
  import torch  # (only for the device's compute-unit count)
  return torch.cuda.get_device_properties(0).multi_processor_count


def _ncl():
  n_cu = _n_cu()
  return n_cu // 32 if n_cu >= 32 and n_cu % 32 == 0 and n_cu // 32 <= 16 else 0


def case_limits(n_utt):
  return [CYCLE[(u + PHASE) % len(CYCLE)] for u in range(n_utt)]


def checked_utterances(n_utt, limits):
  """Every utterance of a row with few; of the many-utterance rows every eighth plus every one under limit 1
  (utterances decode independently: a subset is a valid check)."""
  if n_utt <= 40:
    return list(range(n_utt))
  return [u for u in range(n_utt) if u % 8 == 0 or limits[u] == 1]


@functools.lru_cache(maxsize=None)
def case_reference(case, ncl):
  """The bounded reference of the case's checked utterances, and the unbounded oracle decode of all of them."""
  oracle.lib()
  seqs = case.utterances(ncl)
  limits = case_limits(len(seqs))
  look, tau = (1, 1) if case.session else (case.look_ahead, case.test_iteration)
  free = oracle.decode(case.params(), seqs, case.beam, look, tau, n_threads=8)
  model = primed_ref.Model(case.params())
  ref = {}
  for u in checked_utterances(len(seqs), limits):
    if limits[u]:
      ref[u] = limit_ref.decode(model, seqs[u], case.beam, look, tau, limits[u])
    else:   # (no limit: the oracle's own decode, which limit_ref equals bit for bit -- tests/test_limit_host.py)
      ref[u] = {'labels': free['labels'][u], 'score': free['scores'][u], 'beam_scores': free['beam_scores'][u],
                'max_clusters': int(free['max_clusters'][u])}
  return seqs, limits, free, ref


def binds(case, ncl):
  """The checked utterances whose bounded reference differs from the unbounded oracle decode."""
  _, _, free, ref = case_reference(case, ncl)
  return [u for u, r in ref.items()
          if not np.array_equal(r['labels'], free['labels'][u]) or
          not np.array_equal(_bits(r['beam_scores']), _bits(free['beam_scores'][u]))]


def _same_as_reference(labels, scores, beam_scores, ref, what):
  for u, want in ref.items():
    assert np.array_equal(labels[u], want['labels']), '%s: labels differ, utterance %d' % (what, u)
    assert _bits(scores[u:u + 1])[0] == _bits(want['score'])[0], '%s: score, utterance %d' % (what, u)
    assert np.array_equal(_bits(beam_scores[u]), _bits(want['beam_scores'])), '%s: final beam, utterance %d' % (what, u)


def _decode_case(case, ncl):
  seqs, limits, free, ref = case_reference(case, ncl)
  frames, offsets = oracle.pack(seqs)
  dec = _capi.Decoder(case.params())
  try:
    variants = [case.flags, case.flags | _capi.UIS_FLAG_STEPWISE]
    if case.nodedup:
      variants.append(case.flags | _capi.UIS_FLAG_NO_DEDUP)
    for flags in variants:
      out = dec.decode(frames, offsets, case.beam, case.look_ahead, case.test_iteration, max_clusters=case.cap,
                       flags=flags, want_beam_scores=True, limits=limits)
      what = '%s flags %#x' % (case.name, flags)
      assert out['status'] == 0 and not out['overflow'].any(), what
      inst = dec.last_instantiation()
      if flags & _capi.UIS_FLAG_STEPWISE:
        assert inst == ('stepwise',) + case.row[1:3] + (0, 0), (what, inst)
      else:
        assert inst == case.row, (what, inst)
      labels = [out['labels'][offsets[u]:offsets[u + 1]] for u in range(len(seqs))]
      _same_as_reference(labels, out['scores'], out['beam_scores'], ref, what)
      if len(ref) == len(seqs):   # (every utterance has a reference: the largest cluster count is known)
        assert out['stats']['max_clusters_seen'] == max(r['max_clusters'] for r in ref.values()), what
      else:
        # (the others: a bounded utterance holds at most its limit, an unbounded one what the oracle's decode holds)
        rest = [limits[u] or int(free['max_clusters'][u]) for u in range(len(seqs)) if u not in ref]
        assert max(r['max_clusters'] for r in ref.values()) <= out['stats']['max_clusters_seen'] <= max(
            [r['max_clusters'] for r in ref.values()] + rest), what
      # a bounded utterance ends with at most its limit of speakers, whether it has a reference or not
      for u, lim in enumerate(limits):
        assert not lim or labels[u].size == 0 or int(labels[u].max()) < lim, (what, u)
  finally:
    dec.close()


def _run_session(dec, case, seqs, pushes, flags, limits):
  dec.stream_begin(len(seqs), case.beam, max(len(s) for s in seqs), max_clusters=case.cap, flags=flags, limits=limits)
  try:
    assert dec.stream_limits().tolist() == list(limits)
    pos = [0] * len(seqs)
    picks = []
    for take in pushes:
      chunks = [np.asarray(s[p:p + n], dtype=np.float32) if n else None for s, p, n in zip(seqs, pos, take)]
      pos = [p + n for p, n in zip(pos, take)]
      dec.stream_push(chunks)
      picks.append(dec.last_instantiation())
    labels, scores, overflow, status = dec.stream_labels()
    beam = np.empty((len(seqs), case.beam), dtype=np.float32)
    dec._check(dec._lib.uis_last_decode_info(dec._handle, None, beam.ctypes.data_as(_capi._fp)), 'info')  # pylint: disable=protected-access
  finally:
    dec.stream_end()
  assert status == 0 and not overflow.any(), case.name
  return labels, scores, beam, picks


def _session_case(case, ncl):
  seqs, limits, _, ref = case_reference(case, ncl)
  pushes = case.pushes(ncl)
  hp, dp = case.row[1:3]
  dec = _capi.Decoder(case.params())
  try:
    labels, scores, beam, picks = _run_session(dec, case, seqs, pushes, _capi.UIS_FLAG_PERSISTENT, limits)
    assert set(picks) == {case.row}, (case.name, picks)
    _same_as_reference(labels, scores, beam, ref, case.name + ' persistent')
    labels, scores, beam, picks = _run_session(dec, case, seqs, pushes, _capi.UIS_FLAG_STEPWISE, limits)
    assert set(picks) == {('stepwise', hp, dp, 0, 0)}, (case.name, picks)
    _same_as_reference(labels, scores, beam, ref, case.name + ' stepwise')
    labels, scores, beam, picks = _run_session(dec, case, seqs, pushes, 0, limits)
    assert picks[0] == ('k_decode_resident', hp, dp, 0, 0), (case.name, picks)
    _same_as_reference(labels, scores, beam, ref, case.name + ' plain')
  finally:
    dec.close()


@pytest.mark.parametrize('row', ic.ROWS, ids=[ic.row_id(row) for row in ic.ROWS])
def test_a_bounded_decode_on_every_instantiation(row, oracle_lib):
  ncl = _ncl()
  if ncl == 0:
    pytest.skip('no cluster of 32 compute units: the one-launch kernels do not apply')
  if row[4] and _n_cu() != 256:
    pytest.skip('not a whole MI355X')
  for case in ic.CASES[row]:
    # the test cannot pass with the bound ignored: it binds in at least a quarter of the utterances compared
    _, _, _, ref = case_reference(case, ncl)
    bound = binds(case, ncl)
    assert 4 * len(bound) >= len(ref), (case.name, len(bound), len(ref))
    if case.session:
      _session_case(case, ncl)
    else:
      _decode_case(case, ncl)


# ---- 2. regrouping, through the Python entries

def _params():
  return ic._params(256, 512, 1, None, 0, 0.02)   # pylint: disable=protected-access


def _utterances(lengths, seed=40):
  return [np.asarray(s, dtype=np.float64)
          for s in ic._utterances(256, tuple(lengths), seed, False)]   # pylint: disable=protected-access


def _model(beam, look_ahead=1, test_iteration=1, params=None):
  model_args, _, inference_args = uisrnn_amd.parse_arguments([])
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params if params is not None else _params())
  inference_args.beam_size, inference_args.look_ahead, inference_args.test_iteration = beam, look_ahead, test_iteration
  return model, inference_args


_RAGGED = (9, 1, 130, 4, 12, 2, 20, 6, 3, 14, 8)            # unsorted, one of a single frame, one past a slice boundary
_RAGGED_LIMITS = (2, None, 3, 3, 0, 2, None, 1, 4, 2, 1)


@functools.lru_cache(maxsize=None)
def _ragged_reference(beam, look_ahead, test_iteration, lengths, limits):
  oracle.lib()
  seqs = _utterances(lengths)
  return seqs, limit_ref.decode_list(_params(), seqs, beam, look_ahead, test_iteration, list(limits))


def test_every_utterance_under_its_own_limit_through_two_launches(oracle_lib, monkeypatch):
  seqs, ref = _ragged_reference(10, 1, 1, _RAGGED, _RAGGED_LIMITS)
  want = [r.tolist() for r in ref['labels']]
  assert max(ref['max_clusters'][[1, 4, 6]]) > 2, 'no unbounded utterance opens a third cluster'
  monkeypatch.setenv('UIS_SPLIT_MIN_MB', '0')
  monkeypatch.setenv('UIS_SPLIT_FRAMES', '40')
  model, args = _model(10)
  assert model.predict(seqs, args, max_speakers=list(_RAGGED_LIMITS)) == want
  assert model.last_stats['decode_launches'] == 2 and model._single_pass   # pylint: disable=protected-access
  assert model.predict_single(seqs[2], args, max_speakers=3) == want[2]
  assert model.predict(seqs[7], args, max_speakers=1) == want[7]
  # the table rides on the args object too, and the keyword wins
  args.max_speakers = list(_RAGGED_LIMITS)
  assert model.predict(seqs, args) == want
  args.max_speakers = 1
  assert model.predict(seqs, args, max_speakers=list(_RAGGED_LIMITS)) == want
  args.max_speakers = None
  # the overflow retry through the slices: tables of two clusters send the unbounded utterances (and those bounded above
  # two) round again, the 130-frame one among them, so that the retry's subset decodes in two launches too.  (Clusters
  # whose utterances all end inside the first launch hand their tables over as well: the second launch reads every
  # cluster's back.)
  assert ref['max_clusters'][2] > 2
  args.max_clusters = 2
  assert model.predict(seqs, args, max_speakers=list(_RAGGED_LIMITS)) == want
  assert not model._single_pass   # pylint: disable=protected-access
  args.max_clusters = 0
  # the shards of parallel_predict (the same device twice)
  assert uisrnn_amd.parallel_predict(model, seqs, args, devices=[0, 0], max_speakers=list(_RAGGED_LIMITS)) == want
  # unbounded it is the oracle's decode as before
  free = oracle_lib.decode(_params(), seqs, 10, 1, 1, n_threads=8)
  assert model.predict(seqs, args) == [r.tolist() for r in free['labels']]


_SHORT = (9, 1, 17, 4, 12, 2, 20, 6, 3, 14, 8)


def test_the_overflow_retry_keeps_every_utterances_limit(oracle_lib):
  """Tables of two clusters send the unbounded utterances (and those bounded above two) round again, with twice the
  room: the subsets decode under their members' limits."""
  seqs, ref = _ragged_reference(10, 1, 1, _SHORT, _RAGGED_LIMITS)
  want = [r.tolist() for r in ref['labels']]
  assert max(ref['max_clusters'][[1, 4, 6]]) > 2, 'no unbounded utterance opens a third cluster'
  model, args = _model(10)
  args.max_clusters = 2
  assert model.predict(seqs, args, max_speakers=list(_RAGGED_LIMITS)) == want
  assert not model._single_pass   # pylint: disable=protected-access
  flagged = model._get_decoder().decode_f64(seqs, 10, 1, 1, max_clusters=2,   # pylint: disable=protected-access
                                            limits=[v or 0 for v in _RAGGED_LIMITS])['overflow']
  # an utterance bounded by the table size or less never sets the overflow word
  assert flagged.any() and not flagged[[0, 5, 7, 9, 10]].any(), flagged


def test_the_level_retry_keeps_every_utterances_limit(oracle_lib):
  lengths, limits = (9, 1, 12, 7, 10), (2, None, 0, 1, 2)
  seqs, ref = _ragged_reference(6, 2, 1, lengths, limits)
  want = [r.tolist() for r in ref['labels']]
  model, args = _model(6, look_ahead=2)
  args.max_clusters = 8
  # the precondition: at 16 hypotheses per level some utterances overflow their window, not all
  dec = model._get_decoder()   # pylint: disable=protected-access
  with pytest.raises(_capi.HipLibraryError) as err:
    dec.decode_f64(seqs, 6, 2, 1, max_clusters=8, level_cap=16, limits=[v or 0 for v in limits])
  assert err.value.status == _capi.UIS_ERR_UNSUPPORTED
  full = (dec.last_overflow() & 2) != 0
  assert full.any() and not full.all(), full
  args.level_cap = 16
  assert model.predict(seqs, args, max_speakers=list(limits)) == want


def test_nbest_posteriors_and_primed_under_a_bound(oracle_lib):
  lengths, limits = (12, 1, 9), (2, 1, 3)
  seqs = _utterances(lengths, seed=41)
  beams = [limit_ref.decode(_params(), s, 6, 1, 1, lim)['beam'] for s, lim in zip(seqs, limits)]
  model, args = _model(6)
  got = model.predict_nbest(seqs, args, max_speakers=list(limits))
  post = model.predict_posteriors(seqs, args, temperature=16.0, max_speakers=list(limits))
  for u, beam in enumerate(beams):
    rows = np.array([h.trace for h in beam], dtype=np.int32).reshape(len(beam), lengths[u])
    scores = np.array([h.score for h in beam], dtype=np.float32)
    assert got[u][0] == rows.tolist() and _bits(got[u][1]).tolist() == _bits(scores).tolist(), u
    conf, change, _ = posterior_ref.posterior(rows, scores, 16.0)
    assert post[u][0] == rows[0].tolist()
    assert np.abs(post[u][1] - conf).max() <= posterior_ref.tolerance(len(beam)), u
    assert np.abs(post[u][2] - change).max() <= posterior_ref.tolerance(len(beam)), u
  # primed: a prefix that already holds three clusters under a bound of two is kept and opens nothing more
  prefixes = [[0, 1, 2, 1], [], [0, 0]]
  primed = model.predict_primed(seqs, prefixes, args, max_speakers=[2, 1, 3])
  for u, prefix in enumerate(prefixes):
    want = limit_ref.primed_decode(_params(), np.asarray(seqs[u], dtype=np.float32), prefix, 6, [2, 1, 3][u])
    assert primed[u] == want['labels'][0].tolist(), u
  assert max(primed[0]) == 2


# ---- 3. sessions

def _walk(seed, n_speakers, segment, n_frames):
  return retire_ref.speaker_walk(seed, 256, n_speakers, segment, n_frames)


def _session_flags():
  flags = [('plain', 0), ('stepwise', _capi.UIS_FLAG_STEPWISE)]
  if _n_cu() == 256:
    flags.append(('persistent', _capi.UIS_FLAG_PERSISTENT))
  return flags


def _beam_of(dec, n_utt, beam):
  info = np.empty((n_utt, beam), dtype=np.float32)
  dec._check(dec._lib.uis_last_decode_info(dec._handle, None, info.ctypes.data_as(_capi._fp)), 'info')  # pylint: disable=protected-access
  return info


def test_any_chunking_is_the_offline_bounded_decode(oracle_lib):
  lengths, limits, beam = (21, 1, 13), [2, 1, 3], 6
  seqs = _utterances(lengths, seed=42)
  model = primed_ref.Model(_params())
  ref = [limit_ref.decode(model, s, beam, 1, 1, lim) for s, lim in zip(seqs, limits)]
  frames, offsets = oracle.pack(seqs)
  dec = _capi.Decoder(_params())
  try:
    off = dec.decode(frames, offsets, beam, 1, 1, want_beam_scores=True, limits=limits)
    for name, flags in _session_flags():
      dec.stream_begin(3, beam, 32, flags=flags, limits=limits)
      try:
        for t0, n in ((0, 1), (1, 7), (8, 2), (10, 16)):
          dec.stream_push([np.asarray(s[t0:t0 + n], dtype=np.float32) if len(s) > t0 else None for s in seqs])
        labels, scores, overflow, status = dec.stream_labels()
        info = _beam_of(dec, 3, beam)
      finally:
        dec.stream_end()
      assert status == 0 and not overflow.any()
      for u in range(3):
        assert np.array_equal(labels[u], ref[u]['labels']), (name, u)
        assert np.array_equal(labels[u], off['labels'][offsets[u]:offsets[u + 1]]), (name, u)
        assert np.array_equal(_bits(info[u]), _bits(ref[u]['beam_scores'])), (name, u)
        assert np.array_equal(_bits(info[u]), _bits(off['beam_scores'][u])), (name, u)
  finally:
    dec.close()


def test_limits_change_mid_stream_and_belong_to_the_slot(oracle_lib):
  beam = 4
  seq = np.asarray(_walk(5, 4, 3, 30), dtype=np.float32)
  other = np.asarray(_walk(6, 3, 4, 12), dtype=np.float32)
  params = _params()
  for name, flags in _session_flags():
    ref = limit_ref.Session(params, beam, limit=1)
    side = limit_ref.Session(params, beam, limit=None)
    dec = _capi.Decoder(params)
    try:
      dec.stream_begin(2, beam, 48, flags=flags, limits=[1, 0])

      def check(what):
        labels, scores, overflow, _ = dec.stream_labels()
        info = _beam_of(dec, 2, beam)
        assert not overflow.any(), what
        for u, r in enumerate((ref, side)):
          assert labels[u].tolist() == r.labels(), (name, what, u)
          assert _bits(info[u]).tolist() == _bits(primed_ref.padded_beam(r.scores(), beam)).tolist(), (name, what, u)

      def push(a, b):
        dec.stream_push([a, b])
        ref.push(a)
        if b is not None:
          side.push(b)

      push(seq[:8], other[:5])
      assert ref.K() == 1
      check('limit 1')
      # raised 1 -> 3
      dec.stream_set_limits([3, 0])
      ref.set_limit(3)
      assert dec.stream_limits().tolist() == [3, 0]
      push(seq[8:17], None)
      k_mid = ref.K()
      assert 1 < k_mid <= 3
      check('raised to 3')
      # lowered below a live K: the hypotheses stay, nothing more opens
      dec.stream_set_limits([1, 2])
      ref.set_limit(1)
      side.set_limit(2)
      push(seq[17:24], other[5:])
      assert ref.K() == k_mid
      check('lowered to 1')
      # all or nothing
      with pytest.raises(_capi.HipLibraryError) as err:
        dec.stream_set_limits([2, 4097])
      assert err.value.status == _capi.UIS_ERR_INVALID_ARG and dec.stream_limits().tolist() == [1, 2]
      # restart keeps the slot's limit
      dec.stream_restart([True, False])
      assert dec.stream_limits().tolist() == [1, 2]
      ref = limit_ref.Session(params, beam, limit=1)
      push(seq[:9], None)
      assert ref.K() == 1
      check('after the restart')
      # an exported utterance decodes on under the target slot's limit
      blob = dec.stream_export(1)
      dec.stream_restart([True, False])
      dec.stream_import(0, blob)
      moved = limit_ref.Session(params, beam, limit=1)
      moved.beam, moved.received = [h.copy() for h in side.beam], side.received
      k_side = side.K()
      dec.stream_push([seq[24:], None])
      moved.push(seq[24:])
      assert moved.K() == k_side
      ref = moved
      check('imported')
    finally:
      dec.stream_end()
      dec.close()


def test_after_a_retirement_a_cluster_opens_again(oracle_lib):
  beam, limit = 4, 3
  seq = np.asarray(_walk(11, 6, 4, 36), dtype=np.float32)
  params = _params()
  ref = limit_ref.Session(params, beam, limit=limit)
  dec = _capi.Decoder(params)
  try:
    dec.stream_begin(1, beam, 40, limits=[limit])
    dec.stream_push([seq[:20]])
    ref.push(seq[:20])
    assert ref.K() == limit
    out, _ = dec.stream_commit([4])
    want, _ = ref.commit(4)
    assert out[0].tolist() == want
    able = ref.retirable()
    assert able, 'nothing to retire: pick another walk'
    res = dec.stream_retire(clusters=[able[:1]])
    ref.retire(able[:1])
    assert int(res['K'][0]) == ref.K() == limit - 1
    dec.stream_push([seq[20:]])
    ref.push(seq[20:])
    assert ref.K() == limit, 'no cluster opened after the retirement'
    nb = dec.stream_nbest(beam)
    cnt = int(nb['counts'][0])
    assert nb['labels'][0][:cnt].tolist() == ref.rows().tolist()
    assert _bits(nb['scores'][0][:cnt]).tolist() == _bits(ref.scores()).tolist()
  finally:
    dec.stream_end()
    dec.close()


# ---- 4. a bounded session never overflows

def test_six_speakers_in_tables_of_four(oracle_lib):
  beam, cap = 4, 4
  seq = np.asarray(_walk(23, 6, 4, 36), dtype=np.float32)
  params = _params()
  dec = _capi.Decoder(params)
  try:
    # the precondition, the parent's behaviour: the overflow word is set
    dec.stream_begin(1, beam, 40, max_clusters=cap)
    dec.stream_push([seq])
    _, _, overflow, status = dec.stream_labels()
    dec.stream_end()
    assert overflow[0] != 0 and status == _capi.UIS_ERR_CLUSTER_CAP
    ref = limit_ref.decode(params, seq, beam, 1, 1, limit=cap)
    assert ref['max_clusters'] == cap
    model, args = _model(beam)
    args.max_clusters = cap
    with model.online(1, args, 40, max_speakers=cap) as session:
      assert session.max_speakers() == [cap]
      for t0 in range(0, len(seq), 5):
        session.push([np.asarray(seq[t0:t0 + 5], dtype=np.float64)])
      assert session.labels()[0] == ref['labels'].tolist()      # (labels() raises on overflow)
      rows, scores = session.nbest()[0]
      assert _bits(scores).tolist() == _bits([h.score for h in ref['beam']]).tolist()
    with model.online_pool(2, args, 40) as pool:
      slot = pool.open('a', max_speakers=cap)
      assert pool._session.max_speakers()[slot] == cap   # pylint: disable=protected-access
      pool.push({'a': np.asarray(seq, dtype=np.float64)})
      assert pool.labels('a') == ref['labels'].tolist()
  finally:
    dec.close()


# ---- 5. other checks

def test_the_score_is_score_labels_of_the_labels(oracle_lib):
  lengths, limits = (14, 9, 1), [2, 1, 3]
  seqs = _utterances(lengths, seed=43)
  frames, offsets = oracle.pack(seqs)
  dec = _capi.Decoder(_params())
  try:
    out = dec.decode(frames, offsets, 6, 1, 1, limits=limits)
    scores = dec.score_labels(frames, offsets, out['labels'])
    assert np.array_equal(_bits(scores), _bits(out['scores']))
  finally:
    dec.close()


@pytest.mark.parametrize('word', [None, 'ffffffff', '7f7f7f7f'])
def test_an_unbounded_decode_after_a_bounded_one(word, oracle_lib, monkeypatch):
  """Nothing depends on what an earlier call left: the limit table is written by every decode."""
  if word is None:
    monkeypatch.delenv('UIS_POISON_WORKSPACE', raising=False)
  else:
    monkeypatch.setenv('UIS_POISON_WORKSPACE', word)
  seqs = _utterances((17, 5, 11), seed=44)
  frames, offsets = oracle.pack(seqs)
  free = oracle_lib.decode(_params(), seqs, 10, 1, 1, n_threads=4)
  assert free['max_clusters'].max() > 1
  fresh = _capi.Decoder(_params())
  used = _capi.Decoder(_params())
  try:
    want = fresh.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    bounded = used.decode(frames, offsets, 10, 1, 1, want_beam_scores=True, limits=[1, 1, 1])
    assert not bounded['labels'].any()
    got = used.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    assert np.array_equal(got['labels'], want['labels'])
    assert np.array_equal(_bits(got['beam_scores']), _bits(want['beam_scores']))
    assert np.array_equal(_bits(got['beam_scores']), _bits(free['beam_scores']))
    # a pending table is consumed by the call it was meant for, also when that call is refused
    used.set_limits([1, 1])
    with pytest.raises(_capi.HipLibraryError) as err:
      used.decode(frames, offsets, 10, 1, 1)
    assert err.value.status == _capi.UIS_ERR_INVALID_ARG
    got = used.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    assert np.array_equal(_bits(got['beam_scores']), _bits(free['beam_scores']))
    used.set_limits([1, 1, 1])
    used.set_limits(None)
    got = used.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    assert np.array_equal(_bits(got['beam_scores']), _bits(free['beam_scores']))
    with pytest.raises(_capi.HipLibraryError):
      used.set_limits([1, -1, 1])
    with pytest.raises(_capi.HipLibraryError):
      used.set_limits([1, 4097, 1])
  finally:
    fresh.close()
    used.close()


def test_a_wide_beam_under_a_small_bound_stays_in_one_launch(oracle_lib):
  seqs = _utterances((12, 1, 9), seed=45)
  ref = limit_ref.decode_list(_params(), seqs, 50, 1, 1, [4, 4, 3])
  model, args = _model(50)
  assert model.predict(seqs, args, max_speakers=[4, 4, 3]) == [r.tolist() for r in ref['labels']]
  one_launch = ('k_decode_rs', 'k_decode_resident', 'k_decode_big', 'k_decode_big<WS>', 'k_decode_small')
  assert model.last_stats['decode_kernel'].split(':')[0] in one_launch, model.last_stats['decode_kernel']
  assert model._single_pass   # pylint: disable=protected-access
  dec = model._get_decoder()   # pylint: disable=protected-access
  info = _beam_of(dec, 3, 50)
  assert np.array_equal(_bits(info), _bits(ref['beam_scores']))
  # without the bound the same beam starts at cap 16 and leaves that path
  model.predict(seqs, args)
  assert model.last_stats['decode_kernel'].split(':')[0] not in one_launch, model.last_stats['decode_kernel']
