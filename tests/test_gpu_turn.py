"""Minimum turn length (uis_min_turn) on the GPU against tests/turn_ref.py, bit for bit: labels, scores, final beam,
overflow flags.

  1. one decode under m = 3 (a few cases: m = 5) per non-persist instantiation of the one-launch decode kernels (every case of
     tests/instantiation_cases.py at its own shapes; tests/turn_cases.py holds the m and the references, and
     tests/test_turn_host.py checks on the CPU that the rule changes labels there), UIS_FLAG_NO_DEDUP where the case says
     so; what ran is asserted: never k_decode_rs or k_decode_big<WS> (the owner-side kernel of the same padded shape
     stands in), every other family at its own row;
  2. per-utterance values, and the rule together with known speakers and max_speakers (an empty beam is compared like
     any other result);
  3. the smallest shapes at which the rule can go wrong: k_decode_small at rnn_depth 1 and 2, look_ahead 1 .. 3 with a
     ragged last window, a one-frame utterance, m larger than the utterance, m = 32767, beam 300 on k_window, the
     launch-per-step path with both selects, UIS_FLAG_NO_DEDUP, a host list decoded in slices, the front end's keyword;
  4. nothing stale: a decode without a table after one with a table under UIS_POISON_WORKSPACE is the oracle's;
  5. the refusals of the C ABI.
Before a device comparison outside the sweep a test checks on the CPU that the rule changes the labels of some utterance
it compares: it errors instead of passing vacuously.
"""

import functools

import numpy as np
import pytest

import instantiation_cases as ic
import golden_util
import known_ref
import turn_cases
import turn_ref
import uisrnn_amd
from oracle import oracle
from uisrnn_amd import _capi

pytestmark = pytest.mark.gpu


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ncl():
  import torch  # (only for the device's compute-unit count)
  n_cu = torch.cuda.get_device_properties(0).multi_processor_count
  return n_cu // 32 if n_cu >= 32 and n_cu % 32 == 0 and n_cu // 32 <= 16 else 0


def _changes(free_labels, ref_labels):
  """How many utterances the rule changes; raises where it changes none."""
  changed = sum(not np.array_equal(a, b) for a, b in zip(free_labels, ref_labels))
  if not changed:
    raise RuntimeError('the rule changes no utterance: the comparison would be vacuous')
  return changed


def _same_as_reference(labels, scores, beam_scores, ref, what):
  for u, want in ref.items():
    assert np.array_equal(labels[u], want['labels']), '%s: labels differ, utterance %d' % (what, u)
    assert _bits(scores[u:u + 1])[0] == _bits(want['score'])[0], '%s: score, utterance %d' % (what, u)
    assert np.array_equal(_bits(beam_scores[u]), _bits(want['beam_scores'])), '%s: final beam, utterance %d' % (what, u)


# ---- 1. the instantiation sweep

def _decode_case(case, ncl):
  case, seqs, ms, _, ref = turn_cases.case_reference(case, ncl)   # (the case as the sweep decodes it: its seed, its m)
  frames, offsets = oracle.pack(seqs)
  dec = _capi.Decoder(case.params())
  try:
    variants = [case.flags] + ([case.flags | _capi.UIS_FLAG_NO_DEDUP] if case.nodedup else [])
    for flags in variants:
      out = dec.decode(frames, offsets, case.beam, case.look_ahead, case.test_iteration, max_clusters=case.cap,
                       flags=flags, want_beam_scores=True, min_turn=ms)
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
  finally:
    dec.close()


_OFFLINE_ROWS = [row for row in ic.ROWS if not row[4]]


@pytest.mark.parametrize('row', _OFFLINE_ROWS, ids=[ic.row_id(row) for row in _OFFLINE_ROWS])
def test_a_decode_under_a_minimum_turn_on_every_instantiation(row, oracle_lib):
  ncl = _ncl()
  if ncl == 0:
    pytest.skip('no cluster of 32 compute units: the one-launch kernels do not apply')
  for case in ic.CASES[row]:
    _decode_case(case, ncl)


# ---- 2. per-utterance values; the rules together

_RS128 = (ic.RS, 128, 128, ic.RS_BASE, 0)


@functools.lru_cache(maxsize=None)
def _nine():
  """The first nine utterances of the rs-H128-D128 exact case, taken at ncl = 8, and the oracle's decode of them."""
  oracle.lib()
  case = ic.CASES[_RS128][0]
  assert case.model == 'exact'
  seqs = case.utterances(8)[:9]
  free = oracle.decode(case.params(), seqs, case.beam, 1, case.test_iteration, n_threads=8)
  return case, seqs, free


def _check_list(params, seqs, beam, look_ahead, test_iteration, flags, ms, want, limits=None, tags=None, cap=0,
                free=None, vacuous_ok=False):
  """One decode of `seqs` under ms (and limits, tags) against turn_ref, every utterance.  `want`: the kernel family, or
  a whole instantiation row.  Returns the reference."""
  ref = turn_ref.decode_list(params, seqs, beam, look_ahead, test_iteration, limits=limits, tags=tags, ms=ms)
  if not vacuous_ok:
    free = free or oracle.decode(params, seqs, beam, look_ahead, test_iteration, n_threads=8)
    _changes(free['labels'], ref['labels'])
  frames, offsets = oracle.pack(seqs)
  dec = _capi.Decoder(params)
  try:
    # (inside a window a level's prefixes hold one cluster more per sub-step than the survivors the reference counts)
    cap = cap or max(int(ref['max_clusters'].max()) + look_ahead - 1, 4)
    out = dec.decode(frames, offsets, beam, look_ahead, test_iteration, max_clusters=cap, flags=flags,
                     want_beam_scores=True, min_turn=ms, limits=limits,
                     speakers=None if tags is None else np.concatenate(tags))
    assert out['status'] == 0 and not out['overflow'].any()
    inst = dec.last_instantiation()
    assert (inst[0] == want) if isinstance(want, str) else (inst == want), inst
    for u in range(len(seqs)):
      assert np.array_equal(out['labels'][offsets[u]:offsets[u + 1]], ref['labels'][u]), u
    assert np.array_equal(_bits(out['scores']), _bits(ref['scores']))
    assert np.array_equal(_bits(out['beam_scores']), _bits(ref['beam_scores']))
  finally:
    dec.close()
  return ref


def test_every_utterance_under_its_own_value(oracle_lib):
  if _ncl() == 0:
    pytest.skip('no cluster of 32 compute units: the one-launch kernels do not apply')
  case, seqs, free = _nine()
  ms = [(0, 2, 3, 5)[u % 4] for u in range(len(seqs))]
  ref = _check_list(case.params(), seqs, case.beam, 1, case.test_iteration, _capi.UIS_FLAG_OWNER_SELECT, ms,
                    (ic.RESIDENT, 128, 128, ic.CLS_NONE, 0), cap=case.cap, free=free)
  for u, out in enumerate(ref['outs']):
    assert out['beam'] and all(turn_ref.rule_holds(h.trace, ms[u]) for h in out['beam']), u
    if ms[u] < 2:   # (no rule: the oracle's utterance)
      assert np.array_equal(out['labels'], free['labels'][u]) and _bits(out['score']) == _bits(free['scores'][u:u + 1])[0]


def test_the_rules_together(oracle_lib):
  """m = 3 with known speakers and max_speakers 3: the rules hold together, and where they contradict each other the
  beam is empty -- labels -1, score +inf -- which is compared like any other result."""
  if _ncl() == 0:
    pytest.skip('no cluster of 32 compute units: the one-launch kernels do not apply')
  case, seqs, free = _nine()
  tags = [known_ref.pattern(u, len(s)) for u, s in enumerate(seqs)]
  ref = _check_list(case.params(), seqs, case.beam, 1, case.test_iteration, _capi.UIS_FLAG_OWNER_SELECT,
                    [3] * len(seqs), (ic.RESIDENT, 128, 128, ic.CLS_NONE, 0), limits=[3] * len(seqs), tags=tags,
                    cap=case.cap, free=free)
  empty = [u for u, out in enumerate(ref['outs']) if not out['beam']]
  assert empty and len(empty) < len(seqs)
  for u in empty:
    assert (ref['labels'][u] == -1).all() and np.isposinf(ref['scores'][u]) and np.isposinf(ref['beam_scores'][u]).all()


# ---- 3. the small shapes

_LENGTHS = (9, 1, 17, 4, 12, 2, 20, 6)
# by utterance: m = 3; a one-frame utterance; m = 3 on the ragged last window; m larger than the utterance's 2 x 4
# steps; m = 2; m = 32767; m = 5; no rule
_MS = (3, 3, 3, 40, 2, 32767, 5, 0)


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2'])
@pytest.mark.parametrize('look_ahead', [1, 2, 3])
def test_the_small_models(name, look_ahead, oracle_lib):
  case = golden_util.load_case(name)
  assert int(case['params']['rnn_hidden_size']) == 8 and int(case['params']['rnn_depth']) == (1 if name == 'tiny_d16' else 2)
  lengths = _LENGTHS   # (17 frames: a ragged last window at look_ahead 2 and 3)
  # (utterance u: the first n frames of the first golden sequence from u on that has them)
  pool = case['seqs']
  seqs = [next(pool[(u + k) % len(pool)] for k in range(len(pool)) if len(pool[(u + k) % len(pool)]) >= n)[:n]
          for u, n in enumerate(lengths)]
  assert [len(s) for s in seqs] == list(lengths)
  ref = _check_list(case['params'], seqs, 4 if look_ahead < 3 else 3, look_ahead, 2, _capi.UIS_FLAG_RESIDENT,
                    list(_MS[:len(seqs)]), 'k_decode_small')
  assert ref['labels'][3].tolist() == [0] * 4   # (m beyond the decode: one speaker)


def _params():
  return ic._params(256, 512, 1, None, 0, 0.02)   # pylint: disable=protected-access


def _utterances(lengths, seed=60):
  return [np.asarray(s, dtype=np.float64)
          for s in ic._utterances(256, tuple(lengths), seed, False)]   # pylint: disable=protected-access


_NO_DEDUP = _capi.UIS_FLAG_NO_DEDUP


@pytest.mark.parametrize('name,flags,look_ahead,beam,family', [
    ('default', 0, 1, 6, ic.RESIDENT), ('no dedup', _NO_DEDUP, 1, 6, ic.RESIDENT),
    ('stepwise', _capi.UIS_FLAG_STEPWISE, 1, 6, 'stepwise'),
    ('stepwise no dedup', _capi.UIS_FLAG_STEPWISE | _NO_DEDUP, 1, 6, 'stepwise'),
    ('generic', _capi.UIS_FLAG_STEPWISE | _capi.UIS_FLAG_GENERIC_SELECT, 1, 6, 'stepwise'),
    ('window', 0, 2, 4, ic.WINDOW), ('stepwise look_ahead 2', _capi.UIS_FLAG_STEPWISE, 2, 4, 'stepwise'),
    ('window look_ahead 3', 0, 3, 3, ic.WINDOW), ('stepwise look_ahead 3', _capi.UIS_FLAG_STEPWISE, 3, 3, 'stepwise'),
    ('beam 300', 0, 1, 300, 'stepwise')])
def test_the_edges_on_the_one_launch_kernels_and_the_launch_per_step_path(name, flags, look_ahead, beam, family, oracle_lib):
  """test_iteration 2: the run crosses the pass boundary.  Beam 300 at look_ahead 1 is beyond the select kernels'
  256, so derive_shape hands every step to the window machinery (k_window); the library reports the launch-per-step
  family for it and no more, so which kernel carried the rule there is not asserted, only the bits (test_iteration 1:
  the reference walks 300 hypotheses a step on the CPU)."""
  if family in (ic.RESIDENT, ic.WINDOW) and _ncl() == 0:
    pytest.skip('no cluster of 32 compute units: the one-launch kernels do not apply')
  lengths = _LENGTHS if look_ahead == 1 and beam < 300 else (9, 1, 17, 4, 8) if beam < 300 else (9, 1, 7, 4, 8)
  _check_list(_params(), _utterances(lengths), beam, look_ahead, 2 if beam < 300 else 1, flags, list(_MS[:len(lengths)]),
              family)


def _model(beam, look_ahead=1, test_iteration=1):
  model_args, _, inference_args = uisrnn_amd.parse_arguments([])
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(_params())
  inference_args.beam_size, inference_args.look_ahead, inference_args.test_iteration = beam, look_ahead, test_iteration
  return model, inference_args


_RAGGED = (9, 1, 130, 4, 12, 2, 20, 6, 3, 14, 8)   # unsorted, one of a single frame, one past a slice boundary
_SHORT = (9, 1, 17, 4, 12, 2, 20, 6, 3, 14, 8)


@functools.lru_cache(maxsize=None)
def _list_reference(beam, lengths):
  oracle.lib()
  seqs = _utterances(lengths)
  free = oracle.decode(_params(), seqs, beam, 1, 1, n_threads=8)
  ref = turn_ref.decode_list(_params(), seqs, beam, 1, 1, ms=[3] * len(seqs))
  _changes(free['labels'], ref['labels'])
  return seqs, free, ref


def _beam_of(dec, n_utt, beam):
  info = np.empty((n_utt, beam), dtype=np.float32)
  dec._check(dec._lib.uis_last_decode_info(dec._handle, None, info.ctypes.data_as(_capi._fp)), 'info')  # pylint: disable=protected-access
  return info


def test_the_keyword_on_the_device(oracle_lib):
  seqs, free, ref = _list_reference(10, _SHORT)
  want = [r.tolist() for r in ref['labels']]
  model, args = _model(10)
  assert model.predict(seqs, args, min_turn=3) == want
  assert model.predict(seqs, args, min_turn=[3] * len(seqs)) == want
  assert model.predict_single(seqs[2], args, min_turn=3) == want[2]
  # 0 and 1 are no rule
  assert model.predict(seqs, args, min_turn=1) == [r.tolist() for r in free['labels']]
  # the overflow retry: tables of two clusters put a hypothesis at K = Kmax; the utterances that need more go round
  # again, with their entries of the table
  assert ref['max_clusters'].max() > 2
  args.max_clusters = 2
  assert model.predict(seqs, args, min_turn=3) == want
  assert not model._single_pass   # pylint: disable=protected-access
  args.max_clusters = 0
  # the shards of parallel_predict (the same device twice); n-best and posteriors take the same table
  assert uisrnn_amd.parallel_predict(model, seqs, args, devices=[0, 0], min_turn=3) == want
  assert [r[0][0] for r in model.predict_nbest(seqs, args, min_turn=3)] == want
  assert [r[0] for r in model.predict_posteriors(seqs, args, min_turn=3)] == want
  # every hypothesis of the final beam obeys the rule, not only the best one
  for labelings, _ in model.predict_nbest(seqs, args, min_turn=3):
    assert all(turn_ref.rule_holds(labels, 3) for labels in labelings)


def test_a_host_list_in_slices_is_the_one_launch(oracle_lib, monkeypatch):
  """The runs survive the hand-over between the resumable launches: they ride in the tables it carries."""
  seqs, _, ref = _list_reference(10, _RAGGED)
  want = [r.tolist() for r in ref['labels']]
  model, args = _model(10)
  monkeypatch.setenv('UIS_NO_SPLIT', '1')
  assert model.predict(seqs, args, min_turn=3) == want
  assert model.last_stats['decode_launches'] == 1
  monkeypatch.delenv('UIS_NO_SPLIT')
  monkeypatch.setenv('UIS_SPLIT_MIN_MB', '0')
  monkeypatch.setenv('UIS_SPLIT_FRAMES', '40')
  assert model.predict(seqs, args, min_turn=3) == want
  assert model.last_stats['decode_launches'] == 2
  assert model.last_stats['decode_kernel'].split(':')[0] == 'k_decode_resident', model.last_stats['decode_kernel']
  info = _beam_of(model._get_decoder(), len(seqs), 10)   # pylint: disable=protected-access
  assert np.array_equal(_bits(info), _bits(ref['beam_scores']))


# ---- 4. nothing stale

def test_a_decode_without_a_table_after_one_with_a_table_under_poison(oracle_lib, monkeypatch):
  """The run bits of the first decode are nowhere in the second: it is the oracle's bit for bit, on the kernel a fresh
  handle runs, and a table of zeros and ones is no table."""
  monkeypatch.setenv('UIS_POISON_WORKSPACE', 'ffffffff')
  seqs, free, ref = _list_reference(10, _SHORT)
  frames, offsets = oracle.pack(seqs)
  fresh = _capi.Decoder(_params())
  used = _capi.Decoder(_params())

  def is_the_oracles(got):
    assert np.array_equal(got['labels'], np.concatenate(free['labels']))
    assert np.array_equal(_bits(got['scores']), _bits(free['scores']))
    assert np.array_equal(_bits(got['beam_scores']), _bits(free['beam_scores']))
    assert not got['overflow'].any()

  try:
    fresh.decode(frames, offsets, 10, 1, 1)
    turned = used.decode(frames, offsets, 10, 1, 1, want_beam_scores=True, min_turn=[3] * len(seqs))
    assert np.array_equal(_bits(turned['beam_scores']), _bits(ref['beam_scores']))
    assert np.array_equal(turned['labels'], np.concatenate(ref['labels']))
    is_the_oracles(used.decode(frames, offsets, 10, 1, 1, want_beam_scores=True))
    assert used.last_instantiation() == fresh.last_instantiation()
    # zeros and ones: the decode without a table, on its kernel
    is_the_oracles(used.decode(frames, offsets, 10, 1, 1, want_beam_scores=True, min_turn=[u % 2 for u in range(len(seqs))]))
    assert used.last_instantiation() == fresh.last_instantiation()
    # the launch-per-step path reads the same words
    used.decode(frames, offsets, 10, 1, 1, flags=_capi.UIS_FLAG_STEPWISE, min_turn=[3] * len(seqs))
    is_the_oracles(used.decode(frames, offsets, 10, 1, 1, want_beam_scores=True, flags=_capi.UIS_FLAG_STEPWISE))
  finally:
    fresh.close()
    used.close()


# ---- 5. the refusals

def test_the_refusals_leave_the_handle_usable(oracle_lib):
  seqs, free, ref = _list_reference(10, _SHORT)
  frames, offsets = oracle.pack(seqs)
  labels = np.concatenate(free['labels'])
  table = [3] * len(seqs)
  dec = _capi.Decoder(_params())

  def refused(call):
    dec.set_min_turn(table)
    with pytest.raises(_capi.HipLibraryError) as err:
      call()
    assert err.value.status == _capi.UIS_ERR_UNSUPPORTED and '(uis_min_turn)' in str(err.value), err.value

  def invalid(call):
    with pytest.raises(_capi.HipLibraryError) as err:
      call()
    assert err.value.status == _capi.UIS_ERR_INVALID_ARG, err.value

  def decodes_without_a_rule():
    got = dec.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    assert np.array_equal(got['labels'], labels) and np.array_equal(_bits(got['beam_scores']), _bits(free['beam_scores']))

  try:
    decodes_without_a_rule()
    # the scoring calls: their labels are given
    refused(lambda: dec.score_labels(frames, offsets, labels))
    scores = dec.score_labels(frames, offsets, labels)   # (the table was consumed: the same call now runs)
    assert np.array_equal(_bits(scores), _bits(free['scores']))
    # a session: its operations read the last-label words as labels
    refused(lambda: dec.stream_begin(len(seqs), 10, 32))
    dec.stream_begin(len(seqs), 10, 32)
    try:
      chunks = [np.asarray(s[:3], dtype=np.float32) for s in seqs]
      refused(lambda: dec.stream_push(chunks))
      dec.stream_push(chunks)
      refused(dec.stream_labels)
      assert dec.stream_labels()[3] == 0
    finally:
      dec.stream_end()
    decodes_without_a_rule()   # (the refused tables are gone)
    # a length that is not the decode's utterance count: refused by the decode, and consumed by it
    dec.set_min_turn(table[:-1])
    invalid(lambda: dec.decode(frames, offsets, 10, 1, 1))
    decodes_without_a_rule()
    # values outside [0, 32767]: refused by the setter, which leaves the pending table as it was
    dec.set_min_turn(table)
    invalid(lambda: dec.set_min_turn([3, -1]))
    invalid(lambda: dec.set_min_turn([32768]))
    got = dec.decode(frames, offsets, 10, 1, 1, want_beam_scores=True)
    assert np.array_equal(_bits(got['beam_scores']), _bits(ref['beam_scores']))
    dec.set_min_turn([32767] * len(seqs))   # (the bound itself is a value)
    dec.set_min_turn(None)                  # (NULL clears a pending table)
    decodes_without_a_rule()
  finally:
    dec.close()
