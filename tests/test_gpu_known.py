"""Known speakers (uis_frame_speakers) on the GPU against tests/known_ref.py, bit for bit: labels, scores, final beam.

  1. one decode under the tag pattern per non-persist instantiation of the one-launch decode kernels (every case of
     tests/instantiation_cases.py at its own shapes), UIS_FLAG_NO_DEDUP where the case says so; what ran is asserted:
     never k_decode_rs or k_decode_big<WS> (the owner-side kernel of the same padded shape stands in), every other
     family at its own row; the same call without a table still reports its own row and its own bits;
  2. the smallest shapes at which the rule can go wrong (a tag at frame 0, tag 127, every cluster bound when a tag is
     first met, that under a max_speakers that forbids the new cluster, test_iteration 2, look_ahead 2 and 3 with a
     ragged last window and a tag on a window's last sub-step only, beam 300, transition_bias and max_speakers together
     with tags) on k_decode_small, on the 256 / 512 model's default kernel and on the launch-per-step path;
  3. the regroupings of the front end on the device (overflow retry at K = Kmax, halves, shards), a host list in slices;
  4. nothing stale: a decode without a table after one with a table, plain and under UIS_POISON_WORKSPACE;
  5. the refusals of the C ABI.
Before any device comparison a test checks on the CPU that the pattern changes the labels of at least a quarter of the
utterances of three frames or more that it compares (changed_share): it errors instead of passing vacuously.
"""

import functools

import numpy as np
import pytest

import bias_ref
import golden_util
import instantiation_cases as ic
import known_ref
import primed_ref
import uisrnn_amd
from oracle import oracle
from uisrnn_amd import _capi

pytestmark = pytest.mark.gpu


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _n_cu():
  import torch  # (only for the device's compute-unit count)
  return torch.cuda.get_device_properties(0).multi_processor_count


def _ncl():
  n_cu = _n_cu()
  return n_cu // 32 if n_cu >= 32 and n_cu % 32 == 0 and n_cu // 32 <= 16 else 0


def changed_share(pairs):
  """pairs: (untagged labels, tagged labels) of the utterances a test compares.  Raises where the tags change fewer
  than a quarter of those of at least three frames."""
  long_ones = [(a, b) for a, b in pairs if len(a) >= 3]
  changed = sum(not np.array_equal(a, b) for a, b in long_ones)
  if not long_ones or 4 * changed < len(long_ones):
    raise RuntimeError('the tags change {} of {} utterances: the comparison would be vacuous'.format(changed, len(long_ones)))
  return changed, len(long_ones)


def checked_utterances(n_utt):
  """As tests/test_gpu_bias.py: every utterance of a row with up to four; of the rows with few every other one and the
  single-frame one; of the many-utterance rows every eighth."""
  if n_utt <= 4:
    return list(range(n_utt))
  if n_utt <= 40:
    return [u for u in range(n_utt) if u % 2 == 0 or u == 1]
  return list(range(0, n_utt, 8))


@functools.lru_cache(maxsize=None)
def case_reference(case, ncl):
  """The case's utterances, their tags, the untagged oracle decode and the tagged reference of the checked ones."""
  oracle.lib()
  seqs = case.utterances(ncl)
  tags = [known_ref.pattern(u, len(s)) for u, s in enumerate(seqs)]
  free = oracle.decode(case.params(), seqs, case.beam, case.look_ahead, case.test_iteration, n_threads=8)
  model = primed_ref.Model(case.params())
  ref = {u: known_ref.decode(model, seqs[u], case.beam, case.look_ahead, case.test_iteration, tags=tags[u])
         for u in checked_utterances(len(seqs))}
  changed_share([(free['labels'][u], r['labels']) for u, r in ref.items()])
  return seqs, tags, free, ref


def _same_as_reference(labels, scores, beam_scores, ref, what):
  for u, want in ref.items():
    assert np.array_equal(labels[u], want['labels']), '%s: labels differ, utterance %d' % (what, u)
    assert _bits(scores[u:u + 1])[0] == _bits(want['score'])[0], '%s: score, utterance %d' % (what, u)
    assert np.array_equal(_bits(beam_scores[u]), _bits(want['beam_scores'])), '%s: final beam, utterance %d' % (what, u)


def _decode_case(case, ncl):
  seqs, tags, _, ref = case_reference(case, ncl)
  frames, offsets = oracle.pack(seqs)
  flat = np.concatenate(tags)
  # (the case's cap is kept: the reference's survivors must fit it, a window's prefixes one more per sub-step)
  need = max(r['max_clusters'] for r in ref.values())
  assert need + case.look_ahead - 1 <= case.cap, (case.name, need, case.cap)
  dec = _capi.Decoder(case.params())
  try:
    plain = dec.decode(frames, offsets, case.beam, case.look_ahead, case.test_iteration, max_clusters=case.cap,
                       flags=case.flags, want_beam_scores=True)
    assert plain['status'] == 0 and dec.last_instantiation() == case.row, (case.name, dec.last_instantiation())
    variants = [case.flags] + ([case.flags | _capi.UIS_FLAG_NO_DEDUP] if case.nodedup else [])
    for flags in variants:
      out = dec.decode(frames, offsets, case.beam, case.look_ahead, case.test_iteration, max_clusters=case.cap,
                       flags=flags, want_beam_scores=True, speakers=flat)
      what = '%s flags %#x' % (case.name, flags)
      # (an utterance without a reference may need more room than the case's tables: its flag is its own)
      assert not out['overflow'][list(ref)].any() and (out['status'] == 0 or out['overflow'].any()), what
      inst = dec.last_instantiation()
      assert inst[0] not in (ic.RS, ic.BIG_WS), (what, inst)
      if case.row[0] in (ic.RS, ic.BIG_WS):   # the owner-side kernel of the same padded shape stands in
        assert inst[0] in (ic.RESIDENT, ic.BIG) and inst[1:3] == case.row[1:3] and inst[4] == 0, (what, inst)
      else:
        assert inst == case.row, (what, inst)
      labels = [out['labels'][offsets[u]:offsets[u + 1]] for u in range(len(seqs))]
      _same_as_reference(labels, out['scores'], out['beam_scores'], ref, what)
    # the same call without a table still reports its own row and its own bits
    again = dec.decode(frames, offsets, case.beam, case.look_ahead, case.test_iteration, max_clusters=case.cap,
                       flags=case.flags, want_beam_scores=True)
    assert dec.last_instantiation() == case.row, case.name
    assert np.array_equal(again['labels'], plain['labels']) and np.array_equal(_bits(again['scores']), _bits(plain['scores']))
    assert np.array_equal(_bits(again['beam_scores']), _bits(plain['beam_scores']))
  finally:
    dec.close()


_OFFLINE_ROWS = [row for row in ic.ROWS if not row[4]]


@pytest.mark.parametrize('row', _OFFLINE_ROWS, ids=[ic.row_id(row) for row in _OFFLINE_ROWS])
def test_a_tagged_decode_on_every_instantiation(row, oracle_lib):
  ncl = _ncl()
  if ncl == 0:
    pytest.skip('no cluster of 32 compute units: the one-launch kernels do not apply')
  for case in ic.CASES[row]:
    _decode_case(case, ncl)


# ---- 2. the small shapes

_LENGTHS = (9, 1, 17, 4, 12, 2, 20, 6)


def _edge_tags(lengths, look_ahead):
  """The tables of the small-shape tests, by utterance: 0 a tag at frame 0, tag 127; 1 a single tagged frame; 2 every
  cluster bound when tag 3 is first met (only the new cluster is allowed); 4 a tag on the last sub-step of a window
  only; the others the pattern."""
  tags = [known_ref.pattern(u, n) for u, n in enumerate(lengths)]
  tags[0] = np.array([127, 0, 0, 5, 0, 127, 0, 5, 0], dtype=np.uint8)[:lengths[0]]
  tags[1] = np.array([127], dtype=np.uint8)
  tags[2] = np.array([1, 2, 1, 2, 3] + [0] * (lengths[2] - 5), dtype=np.uint8)
  last = max(int(look_ahead), 1) - 1
  tags[4] = np.array([(1 + t // 6) if t >= 3 and t % max(int(look_ahead), 1) == last and t % 6 == 5 else 0
                      for t in range(lengths[4])], dtype=np.uint8)
  return tags


def _check_edges(params, seqs, beam, look_ahead, test_iteration, flags, want_family, limits=None, biases=None, cap=0):
  tags = _edge_tags([len(s) for s in seqs], look_ahead)
  free = oracle.decode(params, seqs, beam, look_ahead, test_iteration, n_threads=8)
  ref = known_ref.decode_list(params, seqs, beam, look_ahead, test_iteration, limits=limits, biases=biases, tags=tags)
  if limits is None and biases is None:
    changed_share(list(zip(free['labels'], ref['labels'])))
  # the properties, read off the reference's labels: tag 127 at frame 0 is label 0, the forced opening of utterance 2
  assert ref['labels'][0][0] == 0 and ref['labels'][1].tolist() == [0]
  if limits is None:
    assert ref['labels'][2][:5].tolist() == [0, 1, 0, 1, 2]
  frames, offsets = oracle.pack(seqs)
  dec = _capi.Decoder(params)
  try:
    # (inside a window a level's prefixes hold one cluster more per sub-step than the survivors the reference counts)
    cap = cap or max(int(ref['max_clusters'].max()) + look_ahead - 1, 4)
    out = dec.decode(frames, offsets, beam, look_ahead, test_iteration, max_clusters=cap, flags=flags,
                     want_beam_scores=True, speakers=np.concatenate(tags), limits=limits,
                     bias=None if biases is None else np.concatenate(biases))
    assert out['status'] == 0 and not out['overflow'].any()
    assert dec.last_instantiation()[0] == want_family, dec.last_instantiation()
    for u in range(len(seqs)):
      assert np.array_equal(out['labels'][offsets[u]:offsets[u + 1]], ref['labels'][u]), u
    assert np.array_equal(_bits(out['scores']), _bits(ref['scores']))
    assert np.array_equal(_bits(out['beam_scores']), _bits(ref['beam_scores']))
  finally:
    dec.close()
  return ref


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2'])
@pytest.mark.parametrize('look_ahead', [1, 2, 3])
def test_the_small_models_under_tags(name, look_ahead, oracle_lib):
  case = golden_util.load_case(name)
  assert int(case['params']['rnn_hidden_size']) == 8
  lengths = _LENGTHS if look_ahead < 3 else (9, 1, 17, 4, 8)   # (17 frames: a ragged last window at look_ahead 2 and 3)
  seqs = [case['seqs'][u % len(case['seqs'])][:n] for u, n in enumerate(lengths)]
  _check_edges(case['params'], seqs, 4 if look_ahead < 3 else 3, look_ahead, 2, _capi.UIS_FLAG_RESIDENT, 'k_decode_small')


def _params():
  return ic._params(256, 512, 1, None, 0, 0.02)   # pylint: disable=protected-access


def _utterances(lengths, seed=60):
  return [np.asarray(s, dtype=np.float64)
          for s in ic._utterances(256, tuple(lengths), seed, False)]   # pylint: disable=protected-access


@pytest.mark.parametrize('name,flags,look_ahead,beam,family', [
    ('default', 0, 1, 6, ic.RESIDENT), ('stepwise', _capi.UIS_FLAG_STEPWISE, 1, 6, 'stepwise'),
    ('generic', _capi.UIS_FLAG_STEPWISE | _capi.UIS_FLAG_GENERIC_SELECT, 1, 6, 'stepwise'),
    ('window', 0, 2, 4, ic.WINDOW), ('stepwise look_ahead 2', _capi.UIS_FLAG_STEPWISE, 2, 4, 'stepwise'),
    ('window look_ahead 3', 0, 3, 3, ic.WINDOW), ('stepwise look_ahead 3', _capi.UIS_FLAG_STEPWISE, 3, 3, 'stepwise'),
    ('beam 300', 0, 1, 300, 'stepwise')])
def test_the_edges_on_the_one_launch_kernels_and_the_launch_per_step_path(name, flags, look_ahead, beam, family, oracle_lib):
  """test_iteration 2: the second pass is fully forced at the tagged frames.  Beam 300 at look_ahead 1 is beyond the
  select kernels: k_window decides every step (test_iteration 1)."""
  if family in (ic.RESIDENT, ic.WINDOW) and _ncl() == 0:
    pytest.skip('no cluster of 32 compute units: the one-launch kernels do not apply')
  lengths = _LENGTHS if look_ahead == 1 and beam < 300 else (9, 1, 17, 4, 8) if beam < 300 else (9, 1, 7, 4, 8)
  # (beam 300: one pass -- the reference walks 300 hypotheses a step on the CPU)
  _check_edges(_params(), _utterances(lengths), beam, look_ahead, 2 if beam < 300 else 1, flags, family)


def test_transition_bias_and_max_speakers_together_with_tags(oracle_lib):
  seqs = _utterances(_LENGTHS)
  limits = [3, 0, 3, 2, 0, 2, 4, 3]
  biases = [bias_ref.pattern(u, len(s)) for u, s in enumerate(seqs)]
  for u, b in enumerate(biases):   # (a 0 -- stay -- where the tags of _edge_tags force a change would empty the beam)
    b[np.flatnonzero(_edge_tags([len(s) for s in seqs], 1)[u])] = np.nan
  ref = _check_edges(_params(), seqs, 6, 1, 1, 0, ic.RESIDENT if _ncl() else 'stepwise', limits=limits, biases=biases)
  assert all(len(o['beam']) for o in ref['outs'])
  for u, lim in enumerate(limits):
    assert not lim or ref['labels'][u].max() < lim


def test_a_forbidden_new_cluster_empties_one_beam_and_leaves_the_others(oracle_lib):
  """Utterance 2 meets tag 3 with both clusters bound, under max_speakers 2: no candidate is left."""
  seqs = _utterances(_LENGTHS)
  tags = _edge_tags([len(s) for s in seqs], 1)
  limits = [0, 0, 2, 0, 0, 0, 0, 0]
  ref = known_ref.decode_list(_params(), seqs, 6, 1, 1, limits=limits, tags=tags)
  assert not ref['outs'][2]['beam'] and all(o['beam'] for u, o in enumerate(ref['outs']) if u != 2)
  frames, offsets = oracle.pack(seqs)
  dec = _capi.Decoder(_params())
  try:
    for flags in (0, _capi.UIS_FLAG_STEPWISE):
      out = dec.decode(frames, offsets, 6, 1, 1, max_clusters=8, flags=flags, want_beam_scores=True,
                       speakers=np.concatenate(tags), limits=limits)
      assert (out['labels'][offsets[2]:offsets[3]] == -1).all() and np.isposinf(out['scores'][2])
      assert np.isposinf(out['beam_scores'][2]).all()
      for u in range(len(seqs)):
        assert np.array_equal(out['labels'][offsets[u]:offsets[u + 1]], ref['labels'][u]), u
      assert np.array_equal(_bits(out['scores']), _bits(ref['scores']))
      assert np.array_equal(_bits(out['beam_scores']), _bits(ref['beam_scores']))
  finally:
    dec.close()
  model, args = _model(6)
  with pytest.raises(uisrnn_amd.uisrnn.EmptyBeamError):
    model.predict(seqs[2], args, max_speakers=2, known_speakers=_names(tags[2]))


# ---- 3. the regroupings on the device, a host list in slices

def _model(beam, look_ahead=1, test_iteration=1):
  model_args, _, inference_args = uisrnn_amd.parse_arguments([])
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(_params())
  inference_args.beam_size, inference_args.look_ahead, inference_args.test_iteration = beam, look_ahead, test_iteration
  return model, inference_args


def _names(tags):
  """A tag table as the front end takes it: names for the tags (renumbered there, by first appearance), None for 0."""
  return [None if g == 0 else 'speaker {}'.format(int(g)) for g in tags]


_RAGGED = (9, 1, 130, 4, 12, 2, 20, 6, 3, 14, 8)   # unsorted, one of a single frame, one past a slice boundary
_SHORT = (9, 1, 17, 4, 12, 2, 20, 6, 3, 14, 8)


@functools.lru_cache(maxsize=None)
def _list_reference(beam, lengths):
  oracle.lib()
  seqs = _utterances(lengths)
  tags = [known_ref.pattern(u, len(s)) for u, s in enumerate(seqs)]
  free = oracle.decode(_params(), seqs, beam, 1, 1, n_threads=8)
  ref = known_ref.decode_list(_params(), seqs, beam, 1, 1, tags=tags)
  changed_share(list(zip(free['labels'], ref['labels'])))
  return seqs, tags, ref


def _beam_of(dec, n_utt, beam):
  info = np.empty((n_utt, beam), dtype=np.float32)
  dec._check(dec._lib.uis_last_decode_info(dec._handle, None, info.ctypes.data_as(_capi._fp)), 'info')  # pylint: disable=protected-access
  return info


def test_the_table_follows_the_overflow_retry_the_halves_and_the_shards(oracle_lib, monkeypatch):
  seqs, tags, ref = _list_reference(10, _SHORT)
  names = [_names(t) for t in tags]
  want = [r.tolist() for r in ref['labels']]
  assert ref['max_clusters'].max() > 2
  model, args = _model(10)
  assert model.predict(seqs, args, known_speakers=names) == want
  assert model._single_pass   # pylint: disable=protected-access
  assert model.predict_single(seqs[2], args, known_speakers=names[2]) == want[2]
  assert model.predict(seqs[4], args, known_speakers=names[4]) == want[4]
  # the overflow retry: tables of two clusters put a hypothesis at K = Kmax; the utterances that need more go round
  # again, with their rows of the table
  args.max_clusters = 2
  assert model.predict(seqs, args, known_speakers=names) == want
  assert not model._single_pass   # pylint: disable=protected-access
  args.max_clusters = 0
  # the shards of parallel_predict (the same device twice)
  assert uisrnn_amd.parallel_predict(model, seqs, args, devices=[0, 0], known_speakers=names) == want
  # n-best and posteriors take the same table
  assert [r[0][0] for r in model.predict_nbest(seqs, args, known_speakers=names)] == want
  assert [r[0] for r in model.predict_posteriors(seqs, args, known_speakers=names)] == want
  # the halves after UIS_ERR_OOM: one utterance's state is 170 slots x (256 + 512) floats; room for three
  monkeypatch.setenv('UIS_MAX_STATE_BYTES', str(3.5 * 170 * 768 * 4))
  assert model.predict(seqs, args, known_speakers=names) == want
  assert not model._single_pass   # pylint: disable=protected-access


def test_a_host_list_in_slices_is_the_one_launch(oracle_lib, monkeypatch):
  """The bindings survive the hand-over between the resumable launches: they ride in the tables it carries."""
  seqs, tags, ref = _list_reference(10, _RAGGED)
  names = [_names(t) for t in tags]
  want = [r.tolist() for r in ref['labels']]
  model, args = _model(10)
  monkeypatch.setenv('UIS_NO_SPLIT', '1')
  assert model.predict(seqs, args, known_speakers=names) == want
  assert model.last_stats['decode_launches'] == 1
  monkeypatch.delenv('UIS_NO_SPLIT')
  monkeypatch.setenv('UIS_SPLIT_MIN_MB', '0')
  monkeypatch.setenv('UIS_SPLIT_FRAMES', '40')
  assert model.predict(seqs, args, known_speakers=names) == want
  assert model.last_stats['decode_launches'] == 2
  assert model.last_stats['decode_kernel'].split(':')[0] == 'k_decode_resident', model.last_stats['decode_kernel']
  info = _beam_of(model._get_decoder(), len(seqs), 10)   # pylint: disable=protected-access
  assert np.array_equal(_bits(info), _bits(ref['beam_scores']))


# ---- 4. nothing stale

@pytest.mark.parametrize('word', [None, 'ffffffff'])
def test_an_untagged_decode_after_a_tagged_one(word, oracle_lib, monkeypatch):
  """Nothing depends on what an earlier call left, also under UIS_POISON_WORKSPACE: the table is this call's or none."""
  if word is None:
    monkeypatch.delenv('UIS_POISON_WORKSPACE', raising=False)
  else:
    monkeypatch.setenv('UIS_POISON_WORKSPACE', word)
  seqs, tags, ref = _list_reference(10, _SHORT)
  frames, offsets = oracle.pack(seqs)
  flat = np.concatenate(tags)
  fresh = _capi.Decoder(_params())
  used = _capi.Decoder(_params())
  try:
    want = fresh.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    tagged = used.decode(frames, offsets, 10, 1, 1, want_beam_scores=True, speakers=flat)
    assert np.array_equal(_bits(tagged['beam_scores']), _bits(ref['beam_scores']))
    assert not np.array_equal(tagged['labels'], want['labels'])
    got = used.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    assert np.array_equal(got['labels'], want['labels'])
    assert np.array_equal(_bits(got['beam_scores']), _bits(want['beam_scores']))
    assert used.last_instantiation() == fresh.last_instantiation()
    # an all-zero table is the decode without one, bit for bit
    got = used.decode(frames, offsets, 10, 1, 1, want_beam_scores=True, speakers=np.zeros_like(flat))
    assert np.array_equal(got['labels'], want['labels'])
    assert np.array_equal(_bits(got['beam_scores']), _bits(want['beam_scores']))
    # a pending table is consumed by the call it was meant for, also when that call refuses it for its length
    used.set_frame_speakers(flat[:-1])
    with pytest.raises(_capi.HipLibraryError) as err:
      used.decode(frames, offsets, 10, 1, 1)
    assert err.value.status == _capi.UIS_ERR_INVALID_ARG
    got = used.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    assert np.array_equal(_bits(got['beam_scores']), _bits(want['beam_scores']))
    used.set_frame_speakers(flat)
    used.set_frame_speakers(None)
    got = used.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    assert np.array_equal(_bits(got['beam_scores']), _bits(want['beam_scores']))
    with pytest.raises(_capi.HipLibraryError) as err:
      used.set_frame_speakers([1, 128])
    assert err.value.status == _capi.UIS_ERR_INVALID_ARG
    # (a refused table leaves none pending)
    got = used.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    assert np.array_equal(_bits(got['beam_scores']), _bits(want['beam_scores']))
  finally:
    fresh.close()
    used.close()


# ---- 5. the refusals

def test_the_refusals_leave_the_handle_usable(oracle_lib):
  seqs, tags, ref = _list_reference(10, _SHORT)
  frames, offsets = oracle.pack(seqs)
  flat = np.concatenate(tags)
  labels = np.concatenate(ref['labels'])
  dec = _capi.Decoder(_params())

  def refused(call):
    dec.set_frame_speakers(flat)
    with pytest.raises(_capi.HipLibraryError) as err:
      call()
    assert err.value.status == _capi.UIS_ERR_UNSUPPORTED, err.value

  try:
    want = dec.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    # the scoring calls: their labels are given
    refused(lambda: dec.score_labels(frames, offsets, labels))
    scores = dec.score_labels(frames, offsets, labels)   # (the table was consumed: the same call now runs)
    assert np.array_equal(_bits(scores), _bits(ref['scores']))
    refused(lambda: dec.score_speakers(frames, offsets, labels, int(labels.max()) + 2))
    # (the refused call consumes its other table too: a bias left pending with the tags does not reach the next call)
    dec.set_frame_bias(np.full(len(flat), 0.5))
    refused(lambda: dec.score_labels(frames, offsets, labels))
    assert np.array_equal(_bits(dec.score_labels(frames, offsets, labels)), _bits(ref['scores']))
    # every session call made while a table is pending
    refused(lambda: dec.stream_begin(len(seqs), 10, 32))
    dec.stream_begin(len(seqs), 10, 32)
    try:
      chunks = [np.asarray(s[:3], dtype=np.float32) for s in seqs]
      refused(lambda: dec.stream_push(chunks))
      dec.stream_push(chunks)
      refused(dec.stream_labels)
      got = dec.stream_labels()
      assert got[3] == 0
      # uis_stream_end too: the refused call leaves the session open, and the call after it closes it
      refused(dec.stream_end)
      with pytest.raises(_capi.HipLibraryError) as err:
        dec.stream_begin(len(seqs), 10, 32)
      assert err.value.status == _capi.UIS_ERR_INVALID_ARG   # (a session is still open on this handle)
    finally:
      dec.stream_end()
    # ... and the handle decodes as before, with and without a table
    got = dec.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    assert np.array_equal(got['labels'], want['labels']) and np.array_equal(_bits(got['beam_scores']), _bits(want['beam_scores']))
    got = dec.decode(frames, offsets, 10, 1, 1, want_beam_scores=True, speakers=flat)
    assert np.array_equal(_bits(got['beam_scores']), _bits(ref['beam_scores']))
  finally:
    dec.close()


def test_a_decode_of_two_to_the_24_steps_refuses_a_table(oracle_lib):
  """A cluster's tag shares its block-count word, whose count keeps bits 0 .. 23: a decode with a table must keep
  test_iteration * N below 2^24.  The bound is pinned from both sides without a decode of sixteen million steps:
  UIS_FLAG_DEBUG_SCORES with beam 10 wants more than 1e9 candidate scores at either length, which the library refuses
  -- with a message of its own -- after the step count is checked and before anything is allocated.  So at 2^24 - 1 a
  decode with a table, and at 2^24 a decode without one, get past the step count and meet that refusal instead."""
  seqs = _utterances(_SHORT)
  one = np.asarray(seqs[0][:1], dtype=np.float32)
  off1 = np.array([0, 1], dtype=np.int64)
  frames, offsets = oracle.pack(seqs)
  dbg = _capi.UIS_FLAG_DEBUG_SCORES
  dec = _capi.Decoder(_params())

  def refused(tau, speakers, flags):
    with pytest.raises(_capi.HipLibraryError) as err:
      dec.decode(one, off1, 10, 1, tau, max_clusters=16, flags=flags, speakers=speakers)
    assert err.value.status == _capi.UIS_ERR_UNSUPPORTED, err.value
    return str(err.value)

  try:
    want = dec.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    # at the bound: refused for the step count, with and without the flag, as test_iteration and as frames x passes
    assert 'below 2^24' in refused(1 << 24, [1], 0)
    assert 'below 2^24' in refused(1 << 24, [1], dbg)
    assert 'below 2^24' in refused(1 << 24, [0], dbg)   # (a table, whatever it holds)
    long_one = np.zeros((1 << 12, 256), dtype=np.float32)
    with pytest.raises(_capi.HipLibraryError) as err:
      dec.decode(long_one, np.array([0, 1 << 12], dtype=np.int64), 10, 1, 1 << 12, speakers=np.ones(1 << 12, dtype=np.uint8))
    assert err.value.status == _capi.UIS_ERR_UNSUPPORTED and 'below 2^24' in str(err.value)
    # the table was consumed: the next decode, without one, has the untagged bits
    got = dec.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    assert np.array_equal(got['labels'], want['labels']) and np.array_equal(_bits(got['beam_scores']), _bits(want['beam_scores']))
    # one step below the bound the table is accepted, and without a table the bound itself is
    assert 'UIS_FLAG_DEBUG_SCORES' in refused((1 << 24) - 1, [1], dbg)
    assert 'UIS_FLAG_DEBUG_SCORES' in refused(1 << 24, None, dbg)
    # ... and the handle decodes as before, with and without a table
    got = dec.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    assert np.array_equal(got['labels'], want['labels']) and np.array_equal(_bits(got['beam_scores']), _bits(want['beam_scores']))
    tags = [known_ref.pattern(u, len(s)) for u, s in enumerate(seqs)]
    ref = _list_reference(10, _SHORT)[2]
    got = dec.decode(frames, offsets, 10, 1, 1, want_beam_scores=True, speakers=np.concatenate(tags))
    assert np.array_equal(_bits(got['beam_scores']), _bits(ref['beam_scores']))
  finally:
    dec.close()
