"""uis_speaker_profiles / uis_session_profiles on the GPU: each speaker's mean, counts and residual sums.

1. uis_speaker_profiles against the CPU restatement (tests/profiles_ref.py), bit for bit, on six model shapes and a
   ragged batch around the 256-label staging edge; 66 speakers; an invalid trace between valid ones; NaN and inf frames;
2. identities: the scores are uis_score_labels' (with and without a uis_frame_bias table), the stats are numpy's;
3. nothing else is disturbed: repeated and differently shaped calls, UIS_POISON_WORKSPACE, the other scoring calls and a
   decode before and after;
4. sessions: after every push, on every session path and in three chunkings, uis_session_profiles is
   uis_speaker_profiles of the frames received so far under stream_labels(); commit, retire, restart, blobs;
5. the Python front end.

Every float comparison is on uint32 views.
"""

import ctypes
import functools
import os

import numpy as np
import pytest

import golden_util
import profiles_ref
import speakers_ref
import test_gpu_call_tables as gc
import test_gpu_hostile as gh
import test_gpu_retire as gr
import uisrnn_amd
from oracle import oracle
from uisrnn_amd import _capi, synth, weights

pytestmark = pytest.mark.gpu

MODELS = ('toy_d2_depth2', 'tiny_d16', 'd20_h24_depth3', 'tracker_d64_h300', 'trained_d256', 'trained_d512')
WORDS = ('ffffffff', '7f7f7f7f', '80000000')   # test_gpu_poison.py's
KNOB = 'UIS_POISON_WORKSPACE'
FLOATS = ('mean', 'sum_x', 'sum_r2')


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _params(model):
  if model.startswith('trained_'):
    return weights.load_checkpoint(os.path.join(golden_util.GOLDEN_DIR, model + '.uisrnn'))
  return golden_util.load_case(model)['params']


def _cat(labels):
  return np.concatenate(labels).astype(np.int32)


def _ragged_labels():
  """Lengths 1, 2, 3, 40, 255, 256, 257 and 0.  [0, 0, 1] and the 257-frame one end in a cluster whose only frame is the
  utterance's last; the 40-frame one has 18 clusters (the batch's width); the order makes the chains' ranks (longest
  first) differ from their (utterance, cluster) order."""
  long = speakers_ref.revisiting(257, clusters=5)
  long[-1] = 5
  return [np.zeros(1, np.int32), speakers_ref.all_new(2), np.array([0, 0, 1], np.int32), speakers_ref.revisiting(40),
          ((np.arange(255, dtype=np.int32) // 4) % 3).astype(np.int32), speakers_ref.one_cluster(256), long,
          np.zeros(0, np.int32)]


@functools.lru_cache(maxsize=None)
def _batch(model):
  """(seqs, labels, reference profiles) of the ragged batch of one model; the reference is computed once."""
  params = _params(model)
  dim = int(params['observation_dim'])
  labels = _ragged_labels()
  seqs = [synth.make_utterance(9700 + i, max(len(l), 1), dim)[0][:len(l)] for i, l in enumerate(labels)]
  return seqs, labels, profiles_ref.profiles(params, seqs, labels, want_score=False)


def _assert_same(got, want, what):
  assert np.array_equal(got['n_clusters'], want['n_clusters']), (what, got['n_clusters'], want['n_clusters'])
  assert np.array_equal(got['stats'], want['stats']), what
  for key in FLOATS:
    assert got[key].dtype == np.float32 and got[key].shape == want[key].shape, (what, key)
    bad = np.argwhere(_bits(got[key]) != _bits(want[key]))
    assert bad.size == 0, (what, key, bad[:4].tolist(), got[key][tuple(bad[0])], want[key][tuple(bad[0])])


def _check_batch(dec, model, width, what):
  seqs, labels, want = _batch(model)
  frames, offsets = oracle.pack(seqs)
  got = dec.speaker_profiles(frames, offsets, _cat(labels), width)
  _assert_same(got, profiles_ref.padded(want, width, int(_params(model)['observation_dim'])), (what, model, width))
  return got


@pytest.mark.parametrize('model', MODELS)
def test_profiles_match_the_restatement(model):
  _, labels, want = _batch(model)
  assert [p.n_clusters for p in want] == [1, 2, 2, 18, 3, 1, 6, 0]
  assert want[2].stats[1].tolist() == [1, 1, 2, 2] and want[6].stats[5].tolist() == [1, 1, 256, 256]
  dec = _capi.Decoder(_params(model), 0)
  try:
    for width in (18, 21):   # width == K and K + 3
      got = _check_batch(dec, model, width, 'restatement')
    # the identities: score_labels' bits, numpy's stats
    seqs = _batch(model)[0]
    frames, offsets = oracle.pack(seqs)
    assert np.array_equal(_bits(got['scores']), _bits(dec.score_labels(frames, offsets, _cat(labels))))
    for u, l in enumerate(labels):
      assert np.array_equal(got['stats'][u, :want[u].n_clusters], profiles_ref.stats_numpy(l)), u
  finally:
    dec.close()


def test_sixty_six_speakers():
  """One 70-frame utterance with 66 speakers at D 16: more clusters than one 64-thread block."""
  params = _params('tiny_d16')
  labels = np.concatenate([speakers_ref.all_new(66), np.array([3, 65, 65, 0], np.int32)])
  seq = synth.make_utterance(9720, 70, 16)[0]
  want = profiles_ref.profiles(params, [seq], [labels], want_score=False)
  frames, offsets = oracle.pack([seq])
  dec = _capi.Decoder(params, 0)
  try:
    for width in (66, 69):
      _assert_same(dec.speaker_profiles(frames, offsets, labels, width), profiles_ref.padded(want, width, 16), width)
    with pytest.raises(_capi.HipLibraryError, match='width') as err:
      dec.speaker_profiles(frames, offsets, labels, 65)
    assert err.value.status == _capi.UIS_ERR_INVALID_ARG
    _assert_same(dec.speaker_profiles(frames, offsets, labels, 66), profiles_ref.padded(want, 66, 16), 'after the refusal')
  finally:
    dec.close()
  assert want[0].n_clusters == 66 and want[0].stats[65].tolist() == [3, 2, 65, 68]


@pytest.mark.parametrize('model', ['tiny_d16', 'd20_h24_depth3'])
def test_an_invalid_trace_between_two_valid_utterances(model):
  params = _params(model)
  dim = int(params['observation_dim'])
  bad = speakers_ref.invalid_at(40)
  jump = np.array([0, 2, 1, 0, 1], np.int32)
  labels = [speakers_ref.revisiting(12, clusters=4), bad, jump, speakers_ref.one_cluster(9)]
  seqs = [synth.make_utterance(9730 + i, len(l), dim)[0] for i, l in enumerate(labels)]
  want = profiles_ref.profiles(params, seqs, labels, want_score=False)
  assert [p.n_clusters for p in want] == [4, -1, -1, 1]
  frames, offsets = oracle.pack(seqs)
  dec = _capi.Decoder(params, 0)
  try:
    got = dec.speaker_profiles(frames, offsets, _cat(labels), 5)
    _assert_same(got, profiles_ref.padded(want, 5, dim), model)
    assert np.isposinf(got['scores'][1]) and np.isposinf(got['scores'][2]) and np.all(np.isfinite(got['scores'][[0, 3]]))
    # the neighbours are what they are without it
    frames2, offsets2 = oracle.pack([seqs[0], seqs[3]])
    alone = dec.speaker_profiles(frames2, offsets2, _cat([labels[0], labels[3]]), 5)
    for key in FLOATS + ('stats', 'scores'):
      assert np.array_equal(got[key][[0, 3]].view(np.uint32), alone[key].view(np.uint32)), key
  finally:
    dec.close()


def test_non_finite_observations_propagate():
  params = _params('tiny_d16')
  labels = [speakers_ref.revisiting(12, clusters=3), speakers_ref.revisiting(10, clusters=2)]
  seqs = [synth.make_utterance(9740 + i, len(l), 16)[0].copy() for i, l in enumerate(labels)]
  seqs[0][3, 2] = np.nan
  seqs[0][7, 5] = np.inf
  with np.errstate(all='ignore'):
    want = profiles_ref.profiles(params, seqs, labels, want_score=False)
  frames, offsets = oracle.pack(seqs)
  dec = _capi.Decoder(params, 0)
  try:
    got = dec.speaker_profiles(frames, offsets, _cat(labels), 3)
  finally:
    dec.close()
  _assert_same(got, profiles_ref.padded(want, 3, 16), 'non-finite')
  assert np.isnan(got['sum_x'][0]).any() and np.isinf(got['sum_x'][0]).any() and np.all(np.isfinite(got['sum_r2'][1, :2]))


def test_the_bias_table_reaches_the_scores_only():
  params = _params('trained_d256')
  seqs, labels, _ = _batch('trained_d256')
  frames, offsets = oracle.pack(seqs)
  flat = _cat(labels)
  bias = np.random.default_rng(9750).uniform(0.05, 0.95, size=flat.shape[0])
  bias[::7] = np.nan
  dec = _capi.Decoder(params, 0)
  try:
    plain = dec.speaker_profiles(frames, offsets, flat, 18)
    biased = dec.speaker_profiles(frames, offsets, flat, 18, bias=bias)
    want = dec.score_labels(frames, offsets, flat, bias=bias)
    again = dec.speaker_profiles(frames, offsets, flat, 18)   # the table was consumed
  finally:
    dec.close()
  assert np.array_equal(_bits(biased['scores']), _bits(want)) and not np.array_equal(_bits(biased['scores']), _bits(plain['scores']))
  for key in FLOATS + ('stats', 'n_clusters'):
    assert np.array_equal(biased[key].view(np.uint32), plain[key].view(np.uint32)), key
  assert np.array_equal(_bits(again['scores']), _bits(plain['scores']))


@pytest.mark.parametrize('model', ['toy_d2_depth2', 'trained_d256'])
def test_repeated_reshaped_and_poisoned_calls(model, monkeypatch):
  """Two calls give the same bits; a call after a differently shaped one gives a fresh handle's (the restatement's);
  the same under every poison word, where absent rows are zeros and not poison."""
  monkeypatch.delenv(KNOB, raising=False)
  params = _params(model)
  dim = int(params['observation_dim'])
  other = synth.make_utterance(9760, 33, dim)[0]
  oframes, ooffsets = oracle.pack([other, other[:5]])
  olabels = _cat([speakers_ref.revisiting(33, clusters=30), speakers_ref.all_new(5)])
  dec = _capi.Decoder(params, 0)
  try:
    first = _check_batch(dec, model, 21, 'first')
    second = _check_batch(dec, model, 21, 'second')
    for key in FLOATS + ('stats', 'scores'):
      assert np.array_equal(first[key].view(np.uint32), second[key].view(np.uint32)), key
    dec.speaker_profiles(oframes, ooffsets, olabels, 40)
    _check_batch(dec, model, 18, 'after another shape')
    for word in WORDS:
      monkeypatch.setenv(KNOB, word)
      dec.speaker_profiles(oframes, ooffsets, olabels, 31)
      _check_batch(dec, model, 21, 'under ' + word)
  finally:
    dec.close()


def test_the_other_calls_are_what_they_were():
  """uis_score_labels, uis_score_speakers and a decode give identical bits before and after a profiles call."""
  params = _params('trained_d256')
  seqs, labels, _ = _batch('trained_d256')
  frames, offsets = oracle.pack(seqs)
  flat = _cat(labels)
  small = [synth.make_utterance(9770 + i, 30, 256)[0] for i in range(3)]
  sframes, soffsets = oracle.pack(small)

  def others(dec):
    scored = dec.score_labels(frames, offsets, flat, want_frame_losses=True)
    rows = dec.score_speakers(frames, offsets, flat, 19)
    out = dec.decode(sframes, soffsets, 4, 1, 1)
    return [scored[0], scored[1], rows[0], rows[1], out['scores']], out['labels']

  dec = _capi.Decoder(params, 0)
  try:
    before = others(dec)
    dec.speaker_profiles(frames, offsets, flat, 20)
    after = others(dec)
  finally:
    dec.close()
  assert np.array_equal(before[1], after[1])
  for a, b in zip(before[0], after[0]):
    assert np.array_equal(_bits(a), _bits(b))


# ---- the argument checks that precede device work, on a live handle

def _raw(dec, frames, offsets, labels, width, outs):
  """uis_speaker_profiles through ctypes alone: outs = (n_clusters, stats, mean, sum_x, sum_r2, scores), None = NULL."""
  i32p, fp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
  ptr = lambda a, kind: None if a is None else a.ctypes.data_as(kind)
  return dec._lib.uis_speaker_profiles(   # pylint: disable=protected-access
      dec._handle, ptr(frames, fp), ptr(offsets, ctypes.POINTER(ctypes.c_int64)), offsets.shape[0] - 1 if offsets is not None else 1,   # pylint: disable=protected-access
      ptr(labels, i32p), width, ptr(outs[0], i32p), ptr(outs[1], i32p), ptr(outs[2], fp), ptr(outs[3], fp), ptr(outs[4], fp), ptr(outs[5], fp))


def test_null_pointers_and_length_mismatches_on_a_live_handle():
  """Each required pointer as NULL: UIS_ERR_INVALID_ARG and nothing written; the optional outputs as NULL: the others
  are what the full call gives; a bias table or a labels array of another length: refused; the handle goes on working."""
  params = _params('tiny_d16')
  labels = [speakers_ref.revisiting(12, clusters=3), speakers_ref.all_new(2)]
  seqs = [synth.make_utterance(9780 + i, len(l), 16)[0] for i, l in enumerate(labels)]
  frames, offsets = oracle.pack(seqs)
  flat = _cat(labels)
  fresh = lambda: (np.full(2, 77, np.int32), np.full((2, 3, 4), 77, np.int32), np.full((2, 3, 16), 7.0, np.float32),
                   np.full((2, 3, 16), 7.0, np.float32), np.full((2, 3, 16), 7.0, np.float32), np.full(2, 7.0, np.float32))
  untouched = lambda outs: all(o is None or np.all(o == (77 if o.dtype == np.int32 else 7.0)) for o in outs)
  dec = _capi.Decoder(params, 0)
  try:
    full = dec.speaker_profiles(frames, offsets, flat, 3)
    for missing in range(3):   # n_clusters_out, stats_out, mean_out
      outs = list(fresh())
      outs[missing] = None
      assert _raw(dec, frames, offsets, flat, 3, outs) == _capi.UIS_ERR_INVALID_ARG, missing
      assert 'null' in _capi.last_error(dec._lib) and untouched(outs), missing   # pylint: disable=protected-access
    for args in ((None, offsets, flat), (frames, None, flat), (frames, offsets, None)):   # frames, offsets, labels
      outs = fresh()
      assert _raw(dec, args[0], args[1], args[2], 3, outs) == _capi.UIS_ERR_INVALID_ARG
      assert untouched(outs)
    outs = fresh()
    assert _raw(dec, frames, offsets, flat, 2, outs) == _capi.UIS_ERR_INVALID_ARG and untouched(outs)   # width too small
    assert 'width' in _capi.last_error(dec._lib)   # pylint: disable=protected-access
    # the optional outputs, each and all of them absent
    for absent in ((3,), (4,), (5,), (3, 4, 5)):
      outs = list(fresh())
      for i in absent:
        outs[i] = None
      assert _raw(dec, frames, offsets, flat, 3, outs) == _capi.UIS_OK, absent
      for i, key in enumerate(('n_clusters', 'stats', 'mean', 'sum_x', 'sum_r2', 'scores')):
        if outs[i] is not None:
          assert np.array_equal(outs[i].view(np.uint32), full[key].view(np.uint32)), (absent, key)
    # lengths: a bias table of another frame count, labels of another length
    with pytest.raises(_capi.HipLibraryError, match='uis_frame_bias gave 5 ') as err:
      dec.speaker_profiles(frames, offsets, flat, 3, bias=np.full(5, 0.5))
    assert err.value.status == _capi.UIS_ERR_INVALID_ARG
    with pytest.raises(ValueError, match='labels must be'):
      dec.speaker_profiles(frames, offsets, flat[:-1], 3)
    with pytest.raises(ValueError, match='frames must be'):
      dec.speaker_profiles(frames[:-1], offsets, flat, 3)
    again = dec.speaker_profiles(frames, offsets, flat, 3)
    for key in full:
      assert np.array_equal(again[key].view(np.uint32), full[key].view(np.uint32)), key
    # the session call: each output as NULL, then no session at all
    dec.stream_begin(2, 4, 16, max_clusters=4)
    try:
      dec.stream_push(seqs)
      want = dec.stream_profiles()
      i32p, fp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
      for missing in range(3):
        outs = [np.full(2, 77, np.int32), np.full((2, 4, 4), 77, np.int32), np.full((2, 4, 16), 7.0, np.float32)]
        outs[missing] = None
        ptrs = [None if o is None else o.ctypes.data_as(i32p if o.dtype == np.int32 else fp) for o in outs]
        assert dec._lib.uis_session_profiles(dec._handle, 4, *ptrs) == _capi.UIS_ERR_INVALID_ARG, missing   # pylint: disable=protected-access
        assert 'null' in _capi.last_error(dec._lib) and untouched(outs), missing   # pylint: disable=protected-access
      got = dec.stream_profiles()
      for key in want:
        assert np.array_equal(got[key].view(np.uint32), want[key].view(np.uint32)), key
      with pytest.raises(_capi.HipLibraryError, match='streaming session is open'):
        dec.speaker_profiles(frames, offsets, flat, 3)
    finally:
      dec.stream_end()
    with pytest.raises(_capi.HipLibraryError, match='no streaming session'):
      dec.stream_profiles(4)
  finally:
    dec.close()


def test_more_clusters_than_grid_rows_is_refused_before_any_device_work():
  """65536 clusters in one call (one grid row per chain): UIS_ERR_UNSUPPORTED, and the handle goes on working."""
  params = _params('tiny_d16')
  labels = speakers_ref.all_new(65536)
  frames = np.zeros((65536, 16), dtype=np.float32)
  offsets = np.array([0, 65536], dtype=np.int64)
  dec = _capi.Decoder(params, 0)
  try:
    with pytest.raises(_capi.HipLibraryError, match='65535') as err:
      dec.speaker_profiles(frames, offsets, labels, 65536)
    assert err.value.status == _capi.UIS_ERR_UNSUPPORTED
    got = dec.speaker_profiles(frames[:3], offsets // 65536 * 3, labels[:3], 3)
    assert got['n_clusters'].tolist() == [3] and got['stats'][0, :, 0].tolist() == [1, 1, 1]
  finally:
    dec.close()


# ---- the per-call tables: neither entry point is in tests/test_gpu_call_tables.py's table, so its loop runs here

class _ProfilesBench(gc._Bench):   # pylint: disable=protected-access
  def call(self, name):
    if name == 'uis_speaker_profiles':
      self.dec.speaker_profiles(self.frames, self.offsets, self.labels, 2)
    elif name == 'uis_session_profiles':
      self.dec.stream_profiles()
    else:
      super().call(name)


@pytest.mark.parametrize('name,rules,needs', [('uis_speaker_profiles', gc._SCORE, 'none'),   # pylint: disable=protected-access
                                              ('uis_session_profiles', gc._OTHER, 'pushed')])   # pylint: disable=protected-access
def test_the_new_entry_points_follow_their_rules(name, rules, needs):
  """UIS_RULE_SCORE / UIS_RULE_STREAM_OTHER, table by table, as test_every_entry_point_follows_its_rule; then the
  minimum-turn table, which that file's loop does not have: refused, dropped, and the call works afterwards."""
  bench = _ProfilesBench()
  try:
    for table, rule in zip(gc.TABLES, rules):
      what = (name, table)
      bench.prepare(needs)
      bench.set_table(table, gc.WRONG)
      rc, msg = bench.status(bench.call, name)
      if rule == gc.LEAVE:
        assert rc == _capi.UIS_OK, (what, msg)
      elif rule == gc.TAKE:
        assert rc == _capi.UIS_ERR_INVALID_ARG and '{} gave {} '.format(gc.SETTER[table], gc.WRONG) in msg, (what, msg)
      else:
        assert rc == _capi.UIS_ERR_UNSUPPORTED and name + ' takes no ' in msg and '({})'.format(gc.SETTER[table]) in msg, (what, msg)
      assert bench.pending(table) == (rule == gc.LEAVE), what
      bench.clear_tables()
    bench.prepare(needs)
    bench.dec.set_min_turn([3] * gc.N_UTT)
    rc, msg = bench.status(bench.call, name)
    assert rc == _capi.UIS_ERR_UNSUPPORTED and name + ' takes no ' in msg and '(uis_min_turn)' in msg, msg
    assert bench.status(bench.call, name) == (_capi.UIS_OK, '')   # the table was dropped, the handle is usable
  finally:
    bench.clear_tables()
    bench.end()
    bench.dec.close()


# ---- sessions

CHUNKS = (1, 5, 0)   # frames per push; 0: everything at once
LENGTHS = (12, 9, 7)
FLAGS = {'stepwise': _capi.UIS_FLAG_STEPWISE, 'resident': _capi.UIS_FLAG_RESIDENT, 'persistent': _capi.UIS_FLAG_PERSISTENT}
# Which session paths a model takes.  tiny_d16 (hidden size 16, padded to 128): streams never run the 128-wide one-launch
# kernel, so UIS_FLAG_RESIDENT and UIS_FLAG_PERSISTENT are refused (asserted below) and the stepwise path is all there
# is.  trained_d256 (D 256, H 512) must take all three; the persistent one on a whole device.
SESSIONS = [('tiny_d16', 'stepwise'), ('trained_d256', 'stepwise'), ('trained_d256', 'resident'), ('trained_d256', 'persistent')]


def _begin(dec, path, n_utt, beam, window, cap):
  """Open the session on `path`; a refusal is an error."""
  if path == 'persistent' and not gh._whole_device():   # pylint: disable=protected-access
    pytest.skip('not a whole MI355X')
  dec.stream_begin(n_utt, beam, window, max_clusters=cap, flags=FLAGS[path])


@pytest.mark.parametrize('path', ['resident', 'persistent'])
def test_tiny_d16_takes_the_stepwise_path_only(path):
  dec = _capi.Decoder(_params('tiny_d16'), 0)
  try:
    with pytest.raises(_capi.HipLibraryError) as err:
      dec.stream_begin(3, 4, 16, max_clusters=8, flags=FLAGS[path])
    assert err.value.status == _capi.UIS_ERR_UNSUPPORTED
  finally:
    dec.close()


def _check_session(dec, off, received, what, cap=8):
  """uis_session_profiles of `dec` against uis_speaker_profiles (on `off`) of the frames received so far under
  stream_labels(); the tag column against uis_stream_bindings."""
  labels = dec.stream_labels()[0]
  prof = dec.stream_profiles()
  assert prof['stats'].shape == (len(received), cap, 4) and prof['mean'].shape[:2] == (len(received), cap)
  frames, offsets = oracle.pack(received)
  want = off.speaker_profiles(frames, offsets, _cat(labels), cap)
  assert np.array_equal(prof['n_clusters'], want['n_clusters']), (what, prof['n_clusters'], want['n_clusters'])
  assert np.array_equal(prof['stats'][:, :, :2], want['stats'][:, :, :2]), what
  assert np.array_equal(_bits(prof['mean']), _bits(want['mean'])), what
  bindings = dec.stream_bindings()
  for u in range(len(received)):
    k = int(prof['n_clusters'][u])
    assert np.all(prof['stats'][u, k:] == [0, 0, -1, -1]) and np.all(prof['stats'][u, :k, 3] == 0), what
    tags = {int(g): c for c, g in enumerate(prof['stats'][u, :k, 2]) if g > 0}
    assert tags == {g: int(bindings[u, g]) for g in range(1, 128) if bindings[u, g] >= 0}, what
  return prof


@pytest.mark.parametrize('model,path', SESSIONS)
def test_a_session_after_every_push(model, path):
  params = _params(model)
  dim = int(params['observation_dim'])
  seqs = [synth.make_utterance(9800 + u, n, dim)[0] for u, n in enumerate(LENGTHS)]
  off = _capi.Decoder(params, 0)
  try:
    shots = {}
    for chunk in CHUNKS:
      for queried in (True, False):   # (False: the session that is never queried)
        dec = _capi.Decoder(params, 0)
        try:
          _begin(dec, path, 3, 4, 16, 8)
        except BaseException:
          dec.close()
          raise
        try:
          step = chunk or max(LENGTHS)
          for at in range(0, max(LENGTHS), step):
            # tags on the first utterance: the tag column has something to show (a persistent session takes none)
            tags = {}
            sizes = [len(s[at:at + step]) for s in seqs]
            if path != 'persistent':
              table = np.zeros(sum(sizes), dtype=np.uint8)
              table[:sizes[0]] = [1 + ((at + j) // 4) % 2 if (at + j) % 3 == 0 else 0 for j in range(sizes[0])]
              tags = {'speakers': table}
            dec.stream_push([s[at:at + step] if len(s) > at else None for s in seqs], **tags)
            if queried:
              blobs = [dec.stream_export(u) for u in range(3)]
              _check_session(dec, off, [s[:at + step] for s in seqs], (model, path, chunk, at))
              assert blobs == [dec.stream_export(u) for u in range(3)]
          inst = dec.last_instantiation()
          assert inst[4] == (1 if path == 'persistent' else 0), 'the session is no longer persistent'
          assert (inst[0] == 'stepwise') == (path == 'stepwise'), inst   # the path asked for is the path that ran
          labels, scores, _, _ = dec.stream_labels()
          shots[chunk, queried] = ([l.tolist() for l in labels], _bits(scores).tolist())
        finally:
          dec.stream_end()
          dec.close()
      assert shots[chunk, True] == shots[chunk, False], (model, path, chunk)
  finally:
    off.close()


def test_a_session_across_commit_restart_and_a_dead_beam():
  """tracker_d64_h300: after a commit with a horizon the profiles speak about the whole stream; a restarted slot shows 0
  clusters, one whose beam a non-finite frame emptied -1, and the others are untouched."""
  params = _params(gr.MODEL)
  seq = gr.frames(104, gr.SPEAKERS['old'])
  bad = seq[:3].copy()
  bad[2, 0] = np.inf
  dec, off = _capi.Decoder(params, 0), _capi.Decoder(params, 0)
  try:
    dec.stream_begin(3, 4, 32, max_clusters=8)
    try:
      dec.stream_push([seq[:7], seq[:9], bad])
      before = dec.stream_profiles()
      assert before['n_clusters'][2] == -1   # the emptied beam
      committed, _ = dec.stream_commit([3, 3, 3])
      window = dec.stream_labels()[0]
      whole = [np.concatenate([committed[u], window[u]]).astype(np.int32) for u in range(2)]
      prof = dec.stream_profiles()
      frames, offsets = oracle.pack([seq[:7], seq[:9]])
      want = off.speaker_profiles(frames, offsets, _cat(whole), 8)
      assert np.array_equal(prof['n_clusters'][:2], want['n_clusters']) and prof['n_clusters'][2] == -1
      assert np.array_equal(prof['stats'][:2, :, :2], want['stats'][:, :, :2])
      assert np.array_equal(_bits(prof['mean'][:2]), _bits(want['mean']))
      assert np.all(prof['stats'][2] == [0, 0, -1, -1]) and not _bits(prof['mean'][2]).any()
      for key in ('n_clusters', 'stats', 'mean'):   # the commit moved the window, not the speakers
        assert np.array_equal(prof[key].view(np.uint32), before[key].view(np.uint32)), key
      dec.stream_restart([False, True, True])
      after = dec.stream_profiles(11)   # (a wider table)
      assert after['n_clusters'].tolist() == [int(prof['n_clusters'][0]), 0, 0]
      assert np.array_equal(after['stats'][0, :8], prof['stats'][0]) and np.array_equal(_bits(after['mean'][0, :8]), _bits(prof['mean'][0]))
      assert np.all(after['stats'][1:] == [0, 0, -1, -1]) and not _bits(after['mean'][1:]).any()
      with pytest.raises(_capi.HipLibraryError, match='max_clusters') as err:
        dec.stream_profiles(7)
      assert err.value.status == _capi.UIS_ERR_INVALID_ARG
    finally:
      dec.stream_end()
  finally:
    dec.close()
    off.close()


def test_online_session_profiles_across_a_retirement():
  """OnlineSession.profiles / StreamPool.profiles: ids through the session's stable numbering, names from the bindings;
  after retiring a cluster its id is absent and the others keep theirs."""
  beam, cap = 4, 8
  seq = gr.frames(104, gr.SPEAKERS['old'])
  model, args = gr._online(beam, cap)   # pylint: disable=protected-access
  bad = seq[:3].copy()
  bad[2, 0] = np.inf
  with model.online(3, args, 32) as session:
    session.push([seq[:7], seq[:7], bad], known_speakers=[['ann'] + [None] * 6, None, None])
    first = session.profiles()
    assert first[2] is None
    assert first[0]['names'][0] == 'ann' and first[1]['names'] == [None] * len(first[1]['ids'])
    assert first[1]['ids'] == sorted(set(session.labels()[1])) and first[1]['frames'].sum() == 7
    session.commit([3, 3, 3])
    retired = session.retire([1])[1]
    assert retired, 'the scenario retires a cluster'
    second = session.profiles()
    assert second[2] is None and set(second[1]['ids']) == set(first[1]['ids']) - set(retired)
    for c in second[1]['ids']:
      a, b = first[1]['ids'].index(c), second[1]['ids'].index(c)
      assert first[1]['frames'][a] == second[1]['frames'][b] and first[1]['blocks'][a] == second[1]['blocks'][b]
      assert np.array_equal(_bits(first[1]['mean'][a]), _bits(second[1]['mean'][b]))
    for key in ('ids', 'names'):
      assert first[0][key] == second[0][key]
    assert np.array_equal(_bits(first[0]['mean']), _bits(second[0]['mean']))
  with model.online_pool(2, args, 32) as pool:
    pool.open('a')
    pool.push({'a': seq[:7]})
    got = pool.profiles('a')
    assert got['ids'] == first[1]['ids'] and np.array_equal(_bits(got['mean']), _bits(first[1]['mean']))


def test_uisrnn_speaker_profiles_and_sigma2_estimate():
  argv = ['--observation_dim', '256', '--rnn_hidden_size', '512']
  model_args, _, _ = uisrnn_amd.parse_arguments(argv)
  model = uisrnn_amd.UISRNN(model_args)
  model.load(os.path.join(golden_util.GOLDEN_DIR, 'trained_d256.uisrnn'))
  seqs, labels, want = _batch('trained_d256')
  pick = [3, 5, 2]   # 18 clusters, one cluster, [0, 0, 1]
  ids = [['spk{}'.format(c) for c in labels[u]] for u in pick]
  got = model.speaker_profiles([seqs[u] for u in pick], ids)
  assert isinstance(got, list) and all(isinstance(g, uisrnn_amd.SpeakerProfile) for g in got)
  for g, u in zip(got, pick):
    assert g.ids == ['spk{}'.format(k) for k in range(want[u].n_clusters)]
    assert np.array_equal(np.stack([g.frames, g.blocks, g.first, g.last], axis=1), want[u].stats)
    for key in FLOATS:
      assert np.array_equal(_bits(getattr(g, key)), _bits(getattr(want[u], key))), key
    assert g.centroid.dtype == np.float64 and np.array_equal(g.centroid, g.sum_x.astype(np.float64) / g.frames[:, None])
    assert g.score == model.score_labels(seqs[u], ids[pick.index(u)])
  single = model.speaker_profiles(seqs[5], (labels[5] + 7).tolist())
  assert isinstance(single, uisrnn_amd.SpeakerProfile) and single.ids == [7]
  assert np.array_equal(_bits(single.mean), _bits(want[5].mean))
  # sigma2_estimate: the float64 sum over the batch's sum_r2, in list order, over the frames
  total = np.zeros(256, dtype=np.float64)
  for g in got:
    for k in range(len(g.ids)):
      total = total + g.sum_r2[k].astype(np.float64)
  before = np.array(model.sigma2, copy=True)
  sigma2 = model.sigma2_estimate([seqs[u] for u in pick], ids)
  assert sigma2.dtype == np.float64 and np.array_equal(sigma2, total / np.float64(40 + 256 + 3))
  assert np.array_equal(_bits(before), _bits(model.sigma2)) and not np.array_equal(sigma2, before.astype(np.float64))
  dist = uisrnn_amd.speaker_distances(model, got[0], got[1])
  assert dist.shape == (18, 1) and np.all(dist >= 0) and np.all(uisrnn_amd.speaker_distances(model, got[1], got[1]) == 0)
  assert model.last_stats is None
