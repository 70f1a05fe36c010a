"""Per-frame transition_bias on the GPU against tests/bias_ref.py, bit for bit: labels, scores, final beam scores.

  1. one decode under table P per instantiation of the one-launch decode kernels (every case of
     tests/instantiation_cases.py at its own shapes), UIS_FLAG_NO_DEDUP where the case says so; what ran is recorded:
     never k_decode_rs or k_decode_big<WS>, every other family at its own row, k_decode_small on the hidden-8 models;
  2. the launch-per-step path (stepwise, generic select, graph, look_ahead 3) and the host's regroupings (overflow
     retry, UIS_MAX_STATE_BYTES halving, a host list in slices, parallel_predict's shards), max_speakers with a table;
  3. no-table identity: all NaN and all p0 give the bits of the call without a table; poison; nothing stale;
  4. the scoring invariants of DESIGN.md sections 11 / 23 under a table;
  5. sessions through ordinary launches: chunkings, a push without a table after one with, commit / retire / restart /
     export-import between biased pushes, the refusals.
Before any device comparison a test checks on the CPU that table P changes the labels of at least a quarter of the
utterances of three frames or more that it compares (changed_share): it errors instead of passing vacuously.
The reference runs on the CPU: the utterances stay at the case table's lengths.
"""

import functools

import numpy as np
import pytest

import bias_ref
import golden_util
import instantiation_cases as ic
import primed_ref
import retire_ref
import uisrnn_amd
from oracle import oracle
from uisrnn_amd import _capi

pytestmark = pytest.mark.gpu

NAN = float('nan')


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _n_cu():
  import torch  # (only for the device's compute-unit count)
  return torch.cuda.get_device_properties(0).multi_processor_count


def _ncl():
  n_cu = _n_cu()
  return n_cu // 32 if n_cu >= 32 and n_cu % 32 == 0 and n_cu // 32 <= 16 else 0


def changed_share(pairs):
  """pairs: (unbiased labels, biased labels) of the utterances a test compares.  Raises where table P changes fewer
  than a quarter of those of at least three frames."""
  long_ones = [(a, b) for a, b in pairs if len(a) >= 3]
  changed = sum(not np.array_equal(a, b) for a, b in long_ones)
  if not long_ones or 4 * changed < len(long_ones):
    raise RuntimeError('table P changes {} of {} utterances: the comparison would be vacuous'.format(changed, len(long_ones)))
  return changed, len(long_ones)


def checked_utterances(n_utt):
  """Every utterance of a row with up to four; of the rows with few every other one and the single-frame one; of the
  many-utterance rows every eighth.  (Utterances decode independently: a subset is a valid check, and the reference of
  a 512-wide model costs the CPU a second per utterance.)"""
  if n_utt <= 4:
    return list(range(n_utt))
  if n_utt <= 40:
    return [u for u in range(n_utt) if u % 2 == 0 or u == 1]
  return list(range(0, n_utt, 8))


@functools.lru_cache(maxsize=None)
def case_reference(case, ncl):
  """The case's utterances, their tables, the unbiased oracle decode and the biased reference of the checked ones."""
  oracle.lib()
  seqs = case.utterances(ncl)
  tables = [bias_ref.pattern(u, len(s)) for u, s in enumerate(seqs)]
  look, tau = (1, 1) if case.session else (case.look_ahead, case.test_iteration)
  free = oracle.decode(case.params(), seqs, case.beam, look, tau, n_threads=8)
  model = primed_ref.Model(case.params())
  ref = {u: bias_ref.decode(model, seqs[u], case.beam, look, tau, bias=tables[u]) for u in checked_utterances(len(seqs))}
  changed_share([(free['labels'][u], r['labels']) for u, r in ref.items()])
  return seqs, tables, free, ref


def _same_as_reference(labels, scores, beam_scores, ref, what):
  for u, want in ref.items():
    assert np.array_equal(labels[u], want['labels']), '%s: labels differ, utterance %d' % (what, u)
    assert _bits(scores[u:u + 1])[0] == _bits(want['score'])[0], '%s: score, utterance %d' % (what, u)
    assert np.array_equal(_bits(beam_scores[u]), _bits(want['beam_scores'])), '%s: final beam, utterance %d' % (what, u)


def _decode_case(case, ncl):
  seqs, tables, _, ref = case_reference(case, ncl)
  frames, offsets = oracle.pack(seqs)
  flat = np.concatenate(tables)
  # (forced changes open clusters the unbiased decode does not: the tables hold what the reference's survivors need)
  # (three cases' survivors hold more clusters under the table than the case's cap: 9 and 10 against 8, 14 against 12.
  # Their tables grow to what the reference needs -- inside a look-ahead window a level's prefixes open one more per
  # sub-step.  Only rows without a compile-time shape class may grow: the class is keyed on the cap)
  need = max(r['max_clusters'] for r in ref.values())
  cap = case.cap if need <= case.cap else need + case.look_ahead - 1
  assert cap == case.cap or case.row[3] == 0 or case.row[0] == ic.DEEP, (case.name, cap)
  dec = _capi.Decoder(case.params())
  try:
    plain = dec.decode(frames, offsets, case.beam, case.look_ahead, case.test_iteration, max_clusters=case.cap,
                       flags=case.flags)
    assert plain['status'] == 0 and dec.last_instantiation() == case.row, (case.name, dec.last_instantiation())
    variants = [case.flags] + ([case.flags | _capi.UIS_FLAG_NO_DEDUP] if case.nodedup else [])
    for flags in variants:
      out = dec.decode(frames, offsets, case.beam, case.look_ahead, case.test_iteration, max_clusters=cap,
                       flags=flags, want_beam_scores=True, bias=flat)
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
    # the same call without a table still reports its own row, and is not the biased decode
    again = dec.decode(frames, offsets, case.beam, case.look_ahead, case.test_iteration, max_clusters=case.cap,
                       flags=case.flags)
    assert dec.last_instantiation() == case.row, case.name
    assert np.array_equal(again['labels'], plain['labels']) and np.array_equal(_bits(again['scores']), _bits(plain['scores']))
  finally:
    dec.close()


def _beam_of(dec, n_utt, beam):
  info = np.empty((n_utt, beam), dtype=np.float32)
  dec._check(dec._lib.uis_last_decode_info(dec._handle, None, info.ctypes.data_as(_capi._fp)), 'info')  # pylint: disable=protected-access
  return info


def _run_session(dec, case, seqs, tables, pushes, flags):
  dec.stream_begin(len(seqs), case.beam, max(len(s) for s in seqs), max_clusters=case.cap, flags=flags)
  try:
    pos = [0] * len(seqs)
    picks = []
    for take in pushes:
      chunks = [np.asarray(s[p:p + n], dtype=np.float32) if n else None for s, p, n in zip(seqs, pos, take)]
      bias = np.concatenate([t[p:p + n] for t, p, n in zip(tables, pos, take)])
      pos = [p + n for p, n in zip(pos, take)]
      dec.stream_push(chunks, bias=bias)
      picks.append(dec.last_instantiation())
    labels, scores, overflow, status = dec.stream_labels()
    beam = _beam_of(dec, len(seqs), case.beam)
  finally:
    dec.stream_end()
  assert status == 0 and not overflow.any(), case.name
  return labels, scores, beam, picks


def _session_case(case, ncl):
  """The rows of the persist table: a persistent session takes no table (test_the_refusals...), the same session
  through ordinary launches does -- k_decode_resident per push, and the per-step kernels."""
  seqs, tables, _, ref = case_reference(case, ncl)
  pushes = case.pushes(ncl)
  hp, dp = case.row[1:3]
  dec = _capi.Decoder(case.params())
  try:
    labels, scores, beam, picks = _run_session(dec, case, seqs, tables, pushes, 0)
    assert picks[0] == (ic.RESIDENT, hp, dp, 0, 0), (case.name, picks)
    _same_as_reference(labels, scores, beam, ref, case.name + ' plain')
    labels, scores, beam, picks = _run_session(dec, case, seqs, tables, pushes, _capi.UIS_FLAG_STEPWISE)
    assert set(picks) == {('stepwise', hp, dp, 0, 0)}, (case.name, picks)
    _same_as_reference(labels, scores, beam, ref, case.name + ' stepwise')
  finally:
    dec.close()


@pytest.mark.parametrize('row', ic.ROWS, ids=[ic.row_id(row) for row in ic.ROWS])
def test_a_biased_decode_on_every_instantiation(row, oracle_lib):
  ncl = _ncl()
  if ncl == 0:
    pytest.skip('no cluster of 32 compute units: the one-launch kernels do not apply')
  if row[4] and _n_cu() != 256:
    pytest.skip('not a whole MI355X')
  for case in ic.CASES[row]:
    if case.session:
      _session_case(case, ncl)
    else:
      _decode_case(case, ncl)


def test_every_family_but_rs_and_big_ws_has_a_row():
  """test_a_biased_decode_on_every_instantiation asserts, row by row, that the biased decode ran the row's own entry:
  the rows cover resident, big, window and both deep variants (k_decode_small: the next test)."""
  families = {(row[0], row[3]) if row[0] == ic.DEEP else row[0] for row in ic.ROWS if not row[4]}
  assert {ic.RESIDENT, ic.BIG, ic.WINDOW, (ic.DEEP, 0), (ic.DEEP, 1)} <= families


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2'])
@pytest.mark.parametrize('look_ahead', [1, 2])
def test_the_small_models_under_a_table(name, look_ahead, oracle_lib):
  case = golden_util.load_case(name)
  assert int(case['params']['rnn_hidden_size']) == 8
  seqs = [s[:20] for s in case['seqs'][:3]] + [case['seqs'][-1][:1]]
  tables = [bias_ref.pattern(u, len(s)) for u, s in enumerate(seqs)]
  free = oracle_lib.decode(case['params'], seqs, 4, look_ahead, 2, n_threads=4)
  ref = bias_ref.decode_list(case['params'], seqs, 4, look_ahead, 2, biases=tables)
  changed_share(list(zip(free['labels'], ref['labels'])))
  frames, offsets = oracle.pack(seqs)
  dec = _capi.Decoder(case['params'])
  try:
    # (inside a window a level's prefixes hold one cluster more per sub-step than the survivors the reference counts)
    cap = max(int(ref['max_clusters'].max()) + look_ahead - 1, 4)
    out = dec.decode(frames, offsets, 4, look_ahead, 2, max_clusters=cap, flags=_capi.UIS_FLAG_RESIDENT,
                     want_beam_scores=True, bias=np.concatenate(tables))
    assert out['status'] == 0 and out['stats']['decode_kernel'] == 'k_decode_small'
    assert dec.last_instantiation()[0] == 'k_decode_small'
    for u in range(len(seqs)):
      assert np.array_equal(out['labels'][offsets[u]:offsets[u + 1]], ref['labels'][u]), u
    assert np.array_equal(_bits(out['scores']), _bits(ref['scores']))
    assert np.array_equal(_bits(out['beam_scores']), _bits(ref['beam_scores']))
  finally:
    dec.close()


# ---- 2. the launch-per-step path and the regroupings

def _params():
  return ic._params(256, 512, 1, None, 0, 0.02)   # pylint: disable=protected-access


def _utterances(lengths, seed=60):
  return [np.asarray(s, dtype=np.float64)
          for s in ic._utterances(256, tuple(lengths), seed, False)]   # pylint: disable=protected-access


def _model(beam, look_ahead=1, test_iteration=1, params=None):
  model_args, _, inference_args = uisrnn_amd.parse_arguments([])
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params if params is not None else _params())
  inference_args.beam_size, inference_args.look_ahead, inference_args.test_iteration = beam, look_ahead, test_iteration
  return model, inference_args


_RAGGED = (9, 1, 130, 4, 12, 2, 20, 6, 3, 14, 8)   # unsorted, one of a single frame, one past a slice boundary
_SHORT = (9, 1, 17, 4, 12, 2, 20, 6, 3, 14, 8)


@functools.lru_cache(maxsize=None)
def _list_reference(beam, look_ahead, test_iteration, lengths, limits=None, seed=60):
  oracle.lib()
  seqs = _utterances(lengths, seed)
  tables = [bias_ref.pattern(u, len(s)) for u, s in enumerate(seqs)]
  free = oracle.decode(_params(), seqs, beam, look_ahead, test_iteration, n_threads=8)
  ref = bias_ref.decode_list(_params(), seqs, beam, look_ahead, test_iteration, None if limits is None else list(limits), tables)
  changed_share(list(zip(free['labels'], ref['labels'])))
  return seqs, tables, ref


@pytest.mark.parametrize('name,flags,look_ahead', [
    ('stepwise', _capi.UIS_FLAG_STEPWISE, 1), ('generic', _capi.UIS_FLAG_STEPWISE | _capi.UIS_FLAG_GENERIC_SELECT, 1),
    ('graph', _capi.UIS_FLAG_GRAPH, 1), ('stepwise look_ahead 3', _capi.UIS_FLAG_STEPWISE, 3),
    ('graph look_ahead 3', _capi.UIS_FLAG_GRAPH, 3)])
def test_the_launch_per_step_path(name, flags, look_ahead, oracle_lib):
  lengths = _SHORT if look_ahead == 1 else (9, 1, 7, 4, 8)
  beam = 6 if look_ahead == 1 else 3
  seqs, tables, ref = _list_reference(beam, look_ahead, 2, lengths)
  frames, offsets = oracle.pack(seqs)
  dec = _capi.Decoder(_params())
  try:
    cap = max(int(ref['max_clusters'].max()) + look_ahead - 1, 8)
    out = dec.decode(frames, offsets, beam, look_ahead, 2, max_clusters=cap, flags=flags, want_beam_scores=True,
                     bias=np.concatenate(tables))
    assert out['status'] == 0 and dec.last_instantiation()[0] == 'stepwise', (name, dec.last_instantiation())
    for u in range(len(seqs)):
      assert np.array_equal(out['labels'][offsets[u]:offsets[u + 1]], ref['labels'][u]), (name, u)
    assert np.array_equal(_bits(out['scores']), _bits(ref['scores'])), name
    assert np.array_equal(_bits(out['beam_scores']), _bits(ref['beam_scores'])), name
  finally:
    dec.close()


def test_the_table_follows_the_overflow_retry_the_halves_and_the_shards(oracle_lib, monkeypatch):
  seqs, tables, ref = _list_reference(10, 1, 1, _SHORT)
  want = [r.tolist() for r in ref['labels']]
  assert ref['max_clusters'].max() > 2
  model, args = _model(10)
  assert model.predict(seqs, args, transition_bias=tables) == want
  assert model._single_pass   # pylint: disable=protected-access
  assert model.predict_single(seqs[2], args, transition_bias=tables[2]) == want[2]
  assert model.predict(seqs[4], args, transition_bias=tables[4]) == want[4]
  # the overflow retry: tables of two clusters send the utterances that need more round again, with their rows
  args.max_clusters = 2
  assert model.predict(seqs, args, transition_bias=tables) == want
  assert not model._single_pass   # pylint: disable=protected-access
  args.max_clusters = 0
  # the shards of parallel_predict (the same device twice)
  assert uisrnn_amd.parallel_predict(model, seqs, args, devices=[0, 0], transition_bias=tables) == want
  # n-best and posteriors take the same table
  assert [r[0][0] for r in model.predict_nbest(seqs, args, transition_bias=tables)] == want
  assert [r[0] for r in model.predict_posteriors(seqs, args, transition_bias=tables)] == want
  # the halves after UIS_ERR_OOM: one utterance's state is 170 slots x (256 + 512) floats; room for three
  monkeypatch.setenv('UIS_MAX_STATE_BYTES', str(3.5 * 170 * 768 * 4))
  assert model.predict(seqs, args, transition_bias=tables) == want
  assert not model._single_pass   # pylint: disable=protected-access


def test_a_host_list_in_slices_is_the_one_launch(oracle_lib, monkeypatch):
  seqs, tables, ref = _list_reference(10, 1, 1, _RAGGED)
  want = [r.tolist() for r in ref['labels']]
  model, args = _model(10)
  monkeypatch.setenv('UIS_NO_SPLIT', '1')
  assert model.predict(seqs, args, transition_bias=tables) == want
  assert model.last_stats['decode_launches'] == 1
  monkeypatch.delenv('UIS_NO_SPLIT')
  monkeypatch.setenv('UIS_SPLIT_MIN_MB', '0')
  monkeypatch.setenv('UIS_SPLIT_FRAMES', '40')
  assert model.predict(seqs, args, transition_bias=tables) == want
  assert model.last_stats['decode_launches'] == 2
  assert model.last_stats['decode_kernel'].split(':')[0] == 'k_decode_resident', model.last_stats['decode_kernel']
  info = _beam_of(model._get_decoder(), len(seqs), 10)   # pylint: disable=protected-access
  assert np.array_equal(_bits(info), _bits(ref['beam_scores']))


def test_max_speakers_together_with_the_table(oracle_lib):
  limits = (2, None, 3, 3, 0, 2, None, 2, 4, 2, 3)
  seqs, tables, ref = _list_reference(10, 1, 1, _SHORT, limits)
  model, args = _model(10)
  assert model.predict(seqs, args, max_speakers=list(limits), transition_bias=tables) == [r.tolist() for r in ref['labels']]
  info = _beam_of(model._get_decoder(), len(seqs), 10)   # pylint: disable=protected-access
  assert np.array_equal(_bits(info), _bits(ref['beam_scores']))
  for u, lim in enumerate(limits):
    assert not lim or ref['labels'][u].max() < lim
  # a contradiction empties the beam: must change, and no second speaker to change to
  with pytest.raises(uisrnn_amd.uisrnn.EmptyBeamError):
    model.predict(seqs[0], args, max_speakers=1, transition_bias=1.0)
  dec = model._get_decoder()   # pylint: disable=protected-access
  frames, offsets = oracle.pack(seqs[:1])
  out = dec.decode(frames, offsets, 10, 1, 1, limits=[1], bias=np.ones(len(seqs[0])), want_beam_scores=True)
  assert (out['labels'] == -1).all() and np.isposinf(out['scores'][0]) and np.isposinf(out['beam_scores']).all()
  # all stay / all change
  stay = np.zeros(len(seqs[0]))
  stay[0] = NAN
  assert model.predict(seqs[0], args, transition_bias=stay) == [0] * len(seqs[0])
  assert model.predict(seqs[0], args, max_speakers=2, transition_bias=1.0) == [t % 2 for t in range(len(seqs[0]))]


# ---- 3. no-table identity

@pytest.mark.parametrize('name,hidden,depth,beam,look_ahead,flags', [
    ('resident', 512, 1, 8, 1, _capi.UIS_FLAG_OWNER_SELECT), ('window', 512, 1, 4, 2, 0), ('deep', 512, 2, 6, 1, 0),
    ('stepwise', 512, 1, 8, 1, _capi.UIS_FLAG_STEPWISE)])
def test_a_table_without_values_of_its_own_changes_no_bit(name, hidden, depth, beam, look_ahead, flags, oracle_lib):
  params = ic._params(256, hidden, depth, None, 0, 0.02)   # pylint: disable=protected-access
  seqs = _utterances((17, 1, 9, 5, 12), seed=61)
  frames, offsets = oracle.pack(seqs)
  total = int(offsets[-1])
  dec = _capi.Decoder(params)
  try:
    want = dec.decode(frames, offsets, beam, look_ahead, 2, flags=flags, want_beam_scores=True)
    family = dec.last_instantiation()[0]
    if _ncl():
      assert family == {'resident': ic.RESIDENT, 'window': ic.WINDOW, 'deep': ic.DEEP, 'stepwise': 'stepwise'}[name], family
    for what, table in (('all NaN', np.full(total, NAN)), ('all p0', np.full(total, float(params['transition_bias'])))):
      got = dec.decode(frames, offsets, beam, look_ahead, 2, flags=flags, want_beam_scores=True, bias=table)
      assert dec.last_instantiation()[0] == family, (name, what)
      assert np.array_equal(got['labels'], want['labels']), (name, what)
      assert np.array_equal(_bits(got['scores']), _bits(want['scores'])), (name, what)
      assert np.array_equal(_bits(got['beam_scores']), _bits(want['beam_scores'])), (name, what)
  finally:
    dec.close()


@pytest.mark.parametrize('word', [None, 'ffffffff'])
def test_an_unbiased_decode_after_a_biased_one(word, oracle_lib, monkeypatch):
  """Nothing depends on what an earlier call left, also under UIS_POISON_WORKSPACE: the table is this call's or none."""
  if word is None:
    monkeypatch.delenv('UIS_POISON_WORKSPACE', raising=False)
  else:
    monkeypatch.setenv('UIS_POISON_WORKSPACE', word)
  seqs, tables, ref = _list_reference(10, 1, 1, _SHORT)
  frames, offsets = oracle.pack(seqs)
  flat = np.concatenate(tables)
  fresh = _capi.Decoder(_params())
  used = _capi.Decoder(_params())
  try:
    want = fresh.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    biased = used.decode(frames, offsets, 10, 1, 1, want_beam_scores=True, bias=flat)
    assert np.array_equal(_bits(biased['beam_scores']), _bits(ref['beam_scores']))
    assert not np.array_equal(biased['labels'], want['labels'])
    got = used.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    assert np.array_equal(got['labels'], want['labels'])
    assert np.array_equal(_bits(got['beam_scores']), _bits(want['beam_scores']))
    # a pending table is consumed by the call it was meant for, also when that call refuses it for its length
    used.set_frame_bias(flat[:-1])
    with pytest.raises(_capi.HipLibraryError) as err:
      used.decode(frames, offsets, 10, 1, 1)
    assert err.value.status == _capi.UIS_ERR_INVALID_ARG
    got = used.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    assert np.array_equal(_bits(got['beam_scores']), _bits(want['beam_scores']))
    used.set_frame_bias(flat)
    used.set_frame_bias(None)
    got = used.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    assert np.array_equal(_bits(got['beam_scores']), _bits(want['beam_scores']))
    for bad in ([0.5, 1.5], [-0.1], [float('inf')]):
      with pytest.raises(_capi.HipLibraryError) as err:
        used.set_frame_bias(bad)
      assert err.value.status == _capi.UIS_ERR_INVALID_ARG
    # (a refused table leaves none pending)
    got = used.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    assert np.array_equal(_bits(got['beam_scores']), _bits(want['beam_scores']))
  finally:
    fresh.close()
    used.close()


# ---- 4. the scoring invariants under a table

def test_the_score_is_score_labels_of_the_labels(oracle_lib):
  seqs, tables, ref = _list_reference(10, 1, 1, _SHORT)
  model, args = _model(10)
  labels = model.predict(seqs, args, transition_bias=tables)
  scores, losses = model.score_labels(seqs, labels, per_frame=True, transition_bias=tables)
  assert np.array_equal(_bits(scores), _bits(ref['scores']))
  for u, seq in enumerate(seqs):
    want, want_losses = bias_ref.score_one(_params(), seq, labels[u], tables[u])
    assert _bits(want) == _bits(scores[u]) and np.array_equal(_bits(losses[u]), _bits(want_losses)), u
  # without the table the same labels score differently: the keyword reaches the kernel
  assert not np.array_equal(_bits(model.score_labels(seqs, labels)), _bits(scores))
  # a 0 at a change of speaker is a loss of +inf
  hard = [np.zeros(len(s)) for s in seqs]
  got = model.score_labels(seqs[0], labels[0], per_frame=True, transition_bias=hard[0])
  assert np.isposinf(got[0]) and np.isposinf(got[1][0])


def test_score_speakers_is_the_candidate_row_of_a_greedy_decode(oracle_lib):
  """Beam 1: the decode's candidate scores at step t are the score so far plus score_speakers' row t."""
  seqs, tables, _ = _list_reference(10, 1, 1, _SHORT)
  seq, table = seqs[6], tables[6]
  frames, offsets = oracle.pack([seq])
  dec = _capi.Decoder(_params())
  try:
    out = dec.decode(frames, offsets, 1, 1, 1, max_clusters=16, bias=table,
                     flags=_capi.UIS_FLAG_DEBUG_SCORES | _capi.UIS_FLAG_OWNER_SELECT)
    assert out['status'] == 0
    cand = dec.debug_scores(len(seq), 1, 1, 16)[:, 0, 0]   # [steps][17]
    labels = out['labels']
    width = int(labels.max()) + 2
    scores, rows = dec.score_speakers(frames, offsets, labels, width, bias=table)
    assert _bits(scores)[0] == _bits(out['scores'])[0]
    run = np.float32(0.0)
    for t in range(len(seq)):
      want = (run + rows[t]).astype(np.float32)
      assert np.array_equal(_bits(cand[t][:width]), _bits(want)), t
      assert np.isposinf(cand[t][width:]).all()
      run = np.float32(run + rows[t][labels[t]])
    assert np.isposinf(rows[np.flatnonzero(table == 0.0)[0]]).sum() >= 1
  finally:
    dec.close()


# ---- 5. sessions (ordinary launches)

def _walk(seed, n_speakers, segment, n_frames):
  return np.asarray(retire_ref.speaker_walk(seed, 256, n_speakers, segment, n_frames), dtype=np.float32)


_SESSION_FLAGS = (('plain', 0), ('stepwise', _capi.UIS_FLAG_STEPWISE), ('resident', _capi.UIS_FLAG_RESIDENT))


def test_any_chunking_with_per_push_tables_is_the_offline_decode(oracle_lib):
  lengths, beam = (21, 1, 13), 6
  seqs, tables, ref = _list_reference(beam, 1, 1, lengths, seed=62)
  frames, offsets = oracle.pack(seqs)
  dec = _capi.Decoder(_params())
  try:
    off = dec.decode(frames, offsets, beam, 1, 1, want_beam_scores=True, bias=np.concatenate(tables))
    for name, flags in _SESSION_FLAGS:
      if flags == _capi.UIS_FLAG_RESIDENT and not _ncl():
        continue
      dec.stream_begin(3, beam, 32, flags=flags)
      try:
        for t0, n in ((0, 1), (1, 7), (8, 2), (10, 16)):
          dec.stream_push([np.asarray(s[t0:t0 + n], dtype=np.float32) if len(s) > t0 else None for s in seqs],
                          bias=np.concatenate([t[t0:t0 + n] for t in tables]))
        labels, _, overflow, status = dec.stream_labels()
        info = _beam_of(dec, 3, beam)
      finally:
        dec.stream_end()
      assert status == 0 and not overflow.any()
      for u in range(3):
        assert np.array_equal(labels[u], ref['labels'][u]), (name, u)
        assert np.array_equal(labels[u], off['labels'][offsets[u]:offsets[u + 1]]), (name, u)
        assert np.array_equal(_bits(info[u]), _bits(ref['beam_scores'][u])), (name, u)
        assert np.array_equal(_bits(info[u]), _bits(off['beam_scores'][u])), (name, u)
  finally:
    dec.close()


def test_session_operations_between_biased_pushes(oracle_lib):
  """A push with a table, one without, commit, retire, restart and export / import in between; the refusals and a
  table of the wrong length leave the session usable, and the next push runs without a table."""
  beam = 4
  seq = _walk(5, 4, 3, 40)
  other = _walk(6, 3, 4, 16)
  table, side_table = bias_ref.pattern(1, len(seq)), bias_ref.pattern(3, len(other))
  params = _params()
  for name, flags in _SESSION_FLAGS[:2]:
    ref = bias_ref.Session(params, beam)
    side = bias_ref.Session(params, beam)
    dec = _capi.Decoder(params)
    try:
      dec.stream_begin(2, beam, 48, flags=flags)

      def check(what):
        labels, _, overflow, _ = dec.stream_labels()
        info = _beam_of(dec, 2, beam)
        assert not overflow.any(), what
        for u, r in enumerate((ref, side)):
          assert labels[u].tolist() == r.labels(), (name, what, u)
          assert _bits(info[u]).tolist() == _bits(primed_ref.padded_beam(r.scores(), beam)).tolist(), (name, what, u)

      def push(a, b, ta=None, tb=None):
        bias = None
        if ta is not None or tb is not None:
          bias = np.concatenate([np.full(len(a), NAN) if ta is None else ta,
                                 np.zeros(0) if b is None else (np.full(len(b), NAN) if tb is None else tb)])
        dec.stream_push([a, b], bias=bias)
        ref.push(a, ta)
        if b is not None:
          side.push(b, tb)

      push(seq[:8], other[:5], table[:8], side_table[:5])
      check('a push with a table')
      push(seq[8:11], other[5:7])
      check('a push without one')
      push(seq[11:17], None, table[11:17])
      check('one utterance, with a table')
      # a table of the wrong length: refused, consumed, and the next push runs without one
      dec.set_frame_bias(table[:5])
      with pytest.raises(_capi.HipLibraryError) as err:
        dec.stream_push([seq[17:20], None])
      assert err.value.status == _capi.UIS_ERR_INVALID_ARG
      push(seq[17:20], None)
      check('after a refused table')
      # uis_stream_prime refuses a pending table (slot 1 restarted first: priming needs a fresh utterance)
      dec.stream_restart([False, True])
      side = bias_ref.Session(params, beam)
      dec.set_frame_bias(side_table[:4])
      with pytest.raises(_capi.HipLibraryError) as err:
        dec.stream_prime([None, other[:4]], [None, [0, 0, 1, 1]])
      assert err.value.status == _capi.UIS_ERR_UNSUPPORTED
      push(seq[20:22], other[:6], None, side_table[:6])
      check('after the refused priming')
      # commit and retire between biased pushes
      out, _ = dec.stream_commit([4, -1])
      want, _ = ref.commit(4)
      assert out[0].tolist() == want
      able = ref.retirable()
      assert able, 'nothing to retire: pick another walk'
      dec.stream_retire(clusters=[able[:1], []])
      ref.retire(able[:1])
      push(seq[22:30], other[6:10], table[22:30], side_table[6:10])
      nb = dec.stream_nbest(beam)
      cnt = int(nb['counts'][0])
      assert nb['labels'][0][:cnt].tolist() == ref.rows().tolist(), name
      assert _bits(nb['scores'][0][:cnt]).tolist() == _bits(ref.scores()).tolist(), name
      # export / import: slot 1's utterance moves to slot 0 and decodes on under slot 0's rows of the table
      blob = dec.stream_export(1)
      dec.stream_restart([True, False])
      dec.stream_import(0, blob)
      moved = bias_ref.Session(params, beam)
      moved.beam, moved.received = [h.copy() for h in side.beam], side.received
      dec.stream_push([other[10:], None], bias=side_table[10:])
      moved.push(other[10:], side_table[10:])
      labels, _, _, _ = dec.stream_labels()
      assert labels[0].tolist() == moved.labels(), name
      assert _bits(_beam_of(dec, 2, beam)[0]).tolist() == _bits(primed_ref.padded_beam(moved.scores(), beam)).tolist(), name
    finally:
      dec.stream_end()
      dec.close()


def test_a_persistent_session_refuses_a_table_and_goes_on(oracle_lib):
  if _n_cu() != 256:
    pytest.skip('not a whole MI355X')
  beam = 4
  seq = _walk(7, 3, 4, 24)
  table = bias_ref.pattern(0, len(seq))
  params = _params()
  ref = bias_ref.Session(params, beam)
  dec = _capi.Decoder(params)
  try:
    dec.stream_begin(1, beam, 32, flags=_capi.UIS_FLAG_PERSISTENT)
    dec.stream_push([seq[:9]])
    ref.push(seq[:9])
    with pytest.raises(_capi.HipLibraryError) as err:
      dec.stream_push([seq[9:15]], bias=table[9:15])
    assert err.value.status == _capi.UIS_ERR_UNSUPPORTED
    dec.stream_push([seq[9:]])   # (the refused push received nothing; the table is gone)
    ref.push(seq[9:])
    labels, _, overflow, status = dec.stream_labels()
    assert status == 0 and not overflow.any() and labels[0].tolist() == ref.labels()
    assert _bits(_beam_of(dec, 1, beam)[0]).tolist() == _bits(primed_ref.padded_beam(ref.scores(), beam)).tolist()
  finally:
    dec.stream_end()
    dec.close()


def test_the_python_session_takes_the_chunks_layout(oracle_lib):
  beam = 4
  seqs = [np.asarray(_walk(8, 3, 4, 12), dtype=np.float64), np.asarray(_walk(9, 3, 3, 12), dtype=np.float64)]
  tables = [bias_ref.pattern(u, 12) for u in range(2)]
  free = oracle_lib.decode(_params(), seqs, beam, 1, 1, n_threads=2)
  ref = bias_ref.decode_list(_params(), seqs, beam, 1, 1, biases=tables)
  changed_share(list(zip(free['labels'], ref['labels'])))
  want = [r.tolist() for r in ref['labels']]
  model, args = _model(beam)
  with model.online(2, args, 16) as session:
    session.push([seqs[0][:5], seqs[1][:3]], transition_bias=[tables[0][:5], tables[1][:3]])
    session.push([seqs[0][5:7], seqs[1][3:5]], transition_bias=[tables[0][5:7], None])   # (None: the model's)
    assert session.labels()[0] == want[0][:7]
  with model.online(2, args, 16) as session:
    session.push([seqs[0][:5], seqs[1][:3]], transition_bias=[tables[0][:5], tables[1][:3]])
    session.push([seqs[0][5:], seqs[1][3:]], transition_bias=[tables[0][5:], tables[1][3:]])
    assert session.labels() == want
    with pytest.raises(ValueError):
      session.push([seqs[0][:1], None], transition_bias=[[0.5, 0.5], None])
  with model.online(2, args, 16) as session:   # the [U, n, D] form with a [U, n] table
    session.push(np.stack([s[:6] for s in seqs]), transition_bias=np.stack([t[:6] for t in tables]))
    session.push(np.stack([s[6:] for s in seqs]), transition_bias=np.stack([t[6:] for t in tables]))
    assert session.labels() == want
  with model.online_pool(2, args, 16) as pool:
    pool.open('a')
    pool.open('b')
    pool.push({'b': seqs[1], 'a': seqs[0]}, transition_bias={'a': tables[0], 'b': tables[1]})
    assert pool.labels('a') == want[0] and pool.labels('b') == want[1]
