"""Stream export / import on the GPU (uis_stream_export / uis_stream_import): an utterance moved to another slot, and
to a session of another shape on another handle, goes on exactly as it would have where it was.

Every comparison is exact: integer labels and ids, float32 bit patterns.  The reference is the stream's
retire_ref.Session (tests/migrate_plan.py lays out the plans and the cut states on it, before any device call): the
source and both copies are held to the same reference object after every operation, over every readout of
test_gpu_retire.Dev.shot -- labels, scores, the whole beam, overflow, n-best rows and scores, counts, the stable
prefix, committed, the window's frame count, the largest K and the retirable ids.
  1. continuation from every cut state        5. read-only, neighbours
  2. alignment of the records                 6. canonical blobs
  3. other models and session paths           7. refusals
  4. the prior tables                         8. stale memory
"""

import ctypes
import struct

import numpy as np
import pytest

import golden_util
import hostile
import migrate_plan as mp
import test_gpu_hostile as gh
import test_gpu_retire as gt
from uisrnn_amd import _capi

pytestmark = pytest.mark.gpu

WORDS = ('ffffffff', '7f7f7f7f', '80000000')
KNOB = 'UIS_POISON_WORKSPACE'


class Dev(gt.Dev):
  """test_gpu_retire's device session (what OnlineSession keeps: the committed labels, the retired ids), of any model,
  whose utterances can leave and arrive."""

  def __init__(self, params, n_utt, beam, window, cap=16, flags=0):   # pylint: disable=super-init-not-called
    self.dec = _capi.Decoder(params)
    self.dec.stream_begin(n_utt, beam, window, max_clusters=cap, flags=flags)
    self.n, self.beam = n_utt, beam
    self.final = [[] for _ in range(n_utt)]
    self.gone = [[] for _ in range(n_utt)]

  def leave(self, u):
    """The utterance as (the library's blob, the committed labels, the retired ids)."""
    return self.dec.stream_export(u), list(self.final[u]), list(self.gone[u])

  def arrive(self, u, state):
    self.dec.stream_import(u, state[0])
    self.final[u], self.gone[u] = list(state[1]), list(state[2])

  def col(self, u):
    return gt.plain(self.shot())[u]

  def exact(self, u):
    """The columns that must agree between two slots that hold the same stream."""
    return _exact(self.col(u))


def _exact(col):
  return {k: col[k] for k in gt.EXACT}


def _params(name):
  return mp.model(name).params


def _apply(dev, slots, op, frames):
  """One operation of a plan on the slots of `dev` that hold the stream.  Returns its result per slot."""
  kind = op[0]
  if kind == 'push':
    chunks = [None] * dev.n
    for u in slots:
      chunks[u] = frames[op[1]:op[1] + op[2]]
    dev.push(chunks)
    return {u: None for u in slots}
  if kind == 'commit':
    got, dropped = dev.commit([op[1] if u in slots else -1 for u in range(dev.n)])
    return {u: (got[u], dropped[u]) for u in slots}
  if kind == 'retire':
    got, _ = dev.retire([u in slots for u in range(dev.n)])
    return {u: got[u] for u in slots}
  if kind == 'prime':
    chunks, labels = [None] * dev.n, [None] * dev.n
    for u in slots:
      chunks[u], labels[u] = frames[:op[1]], op[2]
    scores = dev.dec.stream_prime(chunks, labels)
    return {u: int(gt._bits(scores)[u]) for u in slots}   # pylint: disable=protected-access
  raise ValueError(op)


def _same(dev, slots, want, what):
  cols = dev.shot()
  for u in slots:
    for key in gt.EXACT:
      assert cols[u][key] == want[key], what + (u, key, cols[u][key], want[key])


def _move(trace, cut, src, other, src_slot=1, dst_slot=4, other_slot=2, dirty=False):
  """The plan of `trace` on slot src_slot of `src`; at the cut the utterance is exported and imported into dst_slot of
  the same session and other_slot of `other`; all three go on to the end of the plan.  dirty: both targets have
  held another stream before and were restarted."""
  frames, at = trace.frames, trace.cuts[cut]['at']
  what = (trace.model_name, trace.beam, cut)
  if dirty:
    junk = frames[::-1][:5]
    src.push([junk if u == dst_slot else None for u in range(src.n)])
    other.push([junk if u == other_slot else None for u in range(other.n)])
  places = [(src, [src_slot])]
  blob = None
  for i, op in enumerate(trace.ops):
    if op[0] == 'cut':
      if i != at:
        continue
      if dirty:
        src.restart({dst_slot})
        other.restart({other_slot})
      before = src.col(src_slot)
      state = src.leave(src_slot)
      blob = state[0]
      assert src.col(src_slot) == before, what + ('export changed the source',)
      src.arrive(dst_slot, state)
      other.arrive(other_slot, state)
      places = [(src, [src_slot, dst_slot]), (other, [other_slot])]
      # canonical: from another slot and from a session of another shape the same bytes come back
      assert src.dec.stream_export(dst_slot) == blob and other.dec.stream_export(other_slot) == blob, what
      assert src.dec.stream_export(src_slot) == blob, what
    for dev, slots in places:   # (one session after the other: a persistent launch has left before the next one starts)
      if op[0] != 'cut':
        got = _apply(dev, slots, op, frames)
        for u in slots:
          assert got[u] == trace.results[i], what + (i, op[0], u, got[u], trace.results[i])
      _same(dev, slots, trace.wants[i], what + (i, op[0]))
  assert blob is not None
  info = _capi.blob_info(blob)
  facts = trace.cuts[cut]
  assert (info['N'], info['committed'], info['live'], info['K']) == (facts['N'], facts['committed'], facts['live'], facts['K']), what
  return blob


def _two(name, beam, window, other_window, other_cap=8, flags=0, n_utt=6, other_n=3):
  return Dev(_params(name), n_utt, beam, window, 16, flags), Dev(_params(name), other_n, beam, other_window, other_cap, flags)


# ---- 1. continuation

CUTS = ('fresh', 'N1', 'N2', 'N3', 'N5', 'full', 'committed', 'emptied')


@pytest.mark.parametrize('beam', [4, 10])
def test_the_cut_states_are_real(beam, oracle_lib):
  cuts = mp.continuation(beam).cuts
  assert [cuts[c]['N'] for c in CUTS[:6]] == [0, 1, 2, 3, 5, 16] and cuts['fresh']['received'] == 0
  assert 1 <= cuts['committed']['live'] < beam and cuts['committed']['committed'] > 0 and cuts['committed']['N'] > 0
  assert cuts['emptied']['N'] == 0 and cuts['emptied']['K'] > 0 and cuts['emptied']['committed'] > 0
  assert cuts['full']['live'] == beam
  start = mp.primed(beam).cuts['primed']
  assert (start['N'], start['committed'], start['live']) == (6, 0, 1)
  old = mp.retired(3)
  assert old.cuts['retired']['gone'] == [0] and old.cuts['retired']['committed'] > 0
  labels = old.wants[-1]['labels']
  assert 4 in labels and 0 not in labels[old.cuts['retired']['received']:]   # speaker 0 came back under a new id


@pytest.mark.parametrize('cut', CUTS)
@pytest.mark.parametrize('beam', [4, 10])
def test_a_moved_stream_continues_as_its_reference(beam, cut, oracle_lib):
  src, other = _two('tiny_d16', beam, 16, 24)
  try:
    _move(mp.continuation(beam), cut, src, other)
  finally:
    src.close()
    other.close()


@pytest.mark.parametrize('beam', [4, 10])
def test_a_primed_stream_moves(beam, oracle_lib):
  src, other = _two('tiny_d16', beam, 16, 24)
  try:
    _move(mp.primed(beam), 'primed', src, other)
  finally:
    src.close()
    other.close()


def test_a_stream_with_retired_clusters_keeps_its_ids(oracle_lib):
  """Renumbered records and a non-empty `gone` travel: the ids after the move are the reference's, the speaker who
  returns gets an id nobody ever had."""
  src, other = _two('tracker_d64_h300', 3, 16, 24, n_utt=6)
  try:
    blob = _move(mp.retired(3), 'retired', src, other)
    assert src.gone[4] == [0] and other.gone[2] == [0] and _capi.blob_info(blob)['committed'] == 4
    assert src.final[4] == src.final[1] and 4 in src.final[4] + src.col(4)['labels']
  finally:
    src.close()
    other.close()


def test_k_exactly_at_the_targets_cap(oracle_lib):
  """Accepted; the next new cluster flags overflow as in any session of that cap that received the same frames; one
  cluster less of room is UIS_ERR_CLUSTER_CAP."""
  trace = mp.at_the_cap(3)
  facts, frames = trace.cuts['at_cap'], trace.frames
  cap = facts['K']
  assert cap >= 4 and trace.wants[-1]['K'] > cap and facts['live'] == 3
  src = Dev(_params(trace.model_name), 2, 3, 16, 16)
  tight = Dev(_params(trace.model_name), 3, 3, 24, cap)
  plain = Dev(_params(trace.model_name), 1, 3, 24, cap)         # "any session": the same frames from the start
  small = Dev(_params(trace.model_name), 1, 3, 24, cap - 1)
  try:
    for i, op in enumerate(trace.ops):
      if op[0] == 'cut':
        state = src.leave(1)
        fresh = small.col(0)
        with pytest.raises(_capi.HipLibraryError) as err:
          small.arrive(0, state)
        assert err.value.status == _capi.UIS_ERR_CLUSTER_CAP and small.col(0) == fresh
        tight.arrive(2, state)
        _same(tight, [2], trace.wants[i], ('at the cap', i))
        continue
      _apply(src, [1], op, frames)
      _apply(plain, [0], op, frames)
      _same(src, [1], trace.wants[i], ('source', i))
      if i > facts['at']:
        _apply(tight, [2], op, frames)
        a, b = tight.exact(2), plain.exact(0)
        assert a == b, ('the copy is not a session of that cap', i, a, b)
    assert tight.col(2)['overflow'] == 1 and src.col(1)['overflow'] == 0
    with pytest.raises(_capi.HipLibraryError) as err:           # an overflowed utterance has nothing to move
      tight.leave(2)
    assert err.value.status == _capi.UIS_ERR_CLUSTER_CAP
  finally:
    for dev in (src, tight, plain, small):
      dev.close()


# ---- 2. alignment

@pytest.mark.parametrize('beam,window', [(3, 15), (4, 16)])
@pytest.mark.parametrize('cut', ['N3', 'N5', 'full', 'committed'])
def test_record_rows_of_any_alignment(beam, window, cut, oracle_lib):
  """Beam 3 at max_frames 15: utterance 1's records start at 180 bytes, utterance 2's at 360 -- neither on a 16-byte
  boundary, and not the same way; the other session's utterance 2 (max_frames 16) starts at 384.  Beam 4 at
  max_frames 16: everything aligned, tails of 0 .. 3 words by N."""
  src, other = _two('tiny_d16', beam, window, 16, n_utt=3)
  assert (window * beam * 4) % 16 == (4 if beam == 3 else 0)
  try:
    _move(mp.continuation(beam, window), cut, src, other, src_slot=1, dst_slot=2, other_slot=2)
  finally:
    src.close()
    other.close()


# ---- 3. other models and session paths

@pytest.mark.parametrize('name,beam', [('toy_d2_depth2', 3), ('tracker_d64_h300', 2)])
@pytest.mark.parametrize('cut', ['odd', 'committed'])
def test_other_model_shapes(name, beam, cut, oracle_lib):
  """Two GRU layers: every layer of pool_hid travels; hidden size 300 embedded in 512: rows in the HidMap layout."""
  for flags in (0, _capi.UIS_FLAG_STEPWISE):
    src, other = _two(name, beam, 16, 24, flags=flags, n_utt=6)
    try:
      _move(mp.short(beam, name), cut, src, other)
    finally:
      src.close()
      other.close()


PATHS = {'default': 0, 'stepwise': _capi.UIS_FLAG_STEPWISE, 'resident': _capi.UIS_FLAG_RESIDENT, 'persistent': _capi.UIS_FLAG_PERSISTENT}


@pytest.mark.parametrize('path', sorted(PATHS))
@pytest.mark.parametrize('cut', ['odd', 'committed'])
def test_the_one_launch_shape_on_every_session_path(path, cut, oracle_lib):
  """persistent: both sessions are; every push goes through a mailbox, the imported utterance's first one included
  (the export that finds the launch resident is test_a_refused_import_costs_a_persistent_session_nothing's)."""
  if path == 'persistent' and not gh._whole_device():   # pylint: disable=protected-access
    pytest.skip('not a whole MI355X')
  src, other = _two('tracker_d256', 3, 16, 24, flags=PATHS[path], n_utt=4)
  try:
    _move(mp.short(3, 'tracker_d256'), cut, src, other, dst_slot=3)
  finally:
    src.close()
    other.close()


# ---- 4. the prior tables / 6. canonical after a long life

def _lines(err, call):
  return [dict(zip(line.split()[1::2], line.split()[2::2])) for line in err.splitlines() if line.startswith(call + ':')]


def test_a_long_stream_brings_its_prior_tables_along(oracle_lib, monkeypatch, capfd):
  """200 frames through a window of 16, then into a session that has just been opened (prior tables of 18 entries):
  the import must lengthen them to committed + N + max_frames + 2 before the next push indexes them."""
  monkeypatch.setenv('UIS_MIGRATE_TRACE', '1')
  trace = mp.endless()
  facts = trace.cuts['long']
  assert facts['committed'] > 10 * 16 and facts['received'] == 200
  src, other = _two('tiny_d16', 4, 16, 16, other_cap=16, n_utt=2, other_n=2)
  try:
    blob = _move(trace, 'long', src, other, src_slot=1, dst_slot=0, other_slot=1)
    again = Dev(_params('tiny_d16'), 5, 4, 20, 12)               # the slots scrambled by 200 steps: still canonical
    again.dec.stream_import(3, blob)
    assert again.dec.stream_export(3) == blob
    again.close()
  finally:
    src.close()
    other.close()
  lines = _lines(capfd.readouterr().err, 'uis_stream_import')
  need = facts['committed'] + facts['N'] + 16 + 2
  assert len(lines) == 3 and int(lines[1]['prior_table_entries']) >= need > 18, lines   # (lines[1]: the just-opened session)
  assert all(int(line['committed']) == facts['committed'] and int(line['window_frames']) == facts['N'] for line in lines)


# ---- 5. read-only, neighbours

def test_export_reads_and_import_leaves_the_neighbours_alone(oracle_lib):
  trace = mp.continuation(4)
  frames = trace.frames
  src, other = _two('tiny_d16', 4, 16, 24, n_utt=4, other_n=3)
  try:
    src.push([frames[:7], frames[3:8], None, frames[10:26]])
    src.commit([2, -1, -1, 8])
    other.push([frames[5:9], None, frames[1:12]])
    other.commit([-1, -1, 4])
    before = gt.plain(src.shot())
    states = [src.leave(u) for u in range(4)]
    assert gt.plain(src.shot()) == before                           # every readout of the source, every utterance
    assert [src.dec.stream_export(u) for u in range(4)] == [s[0] for s in states]
    there = gt.plain(other.shot())
    other.arrive(1, states[3])
    after = gt.plain(other.shot())
    assert after[0] == there[0] and after[2] == there[2] and _exact(after[1]) == _exact(before[3])
    src.restart({2})
    src.arrive(2, states[0])
    now = gt.plain(src.shot())
    assert [now[u] for u in (0, 1, 3)] == [before[u] for u in (0, 1, 3)] and _exact(now[2]) == _exact(before[0])
  finally:
    src.close()
    other.close()


# ---- 7. refusals

def _raw_import(dec, utt, blob, size=None):
  return dec._lib.uis_stream_import(dec._handle, utt, blob, len(blob) if size is None else size)   # pylint: disable=protected-access


def _raw_export(dec, utt, capacity):
  buf = ctypes.create_string_buffer(b'\x55' * max(capacity, 1), max(capacity, 1))
  n = ctypes.c_int64(-7)
  rc = dec._lib.uis_stream_export(dec._handle, utt, buf, capacity, ctypes.byref(n))   # pylint: disable=protected-access
  return rc, n.value, buf.raw


def _refusals(dev, blob, other_model_blob, other_beam_blob, long_blob, big_k_blob):
  """(what, call, status) of everything a session of two utterances -- 0 live, 1 fresh -- must refuse."""
  flipped = bytearray(blob)
  flipped[len(blob) // 2] ^= 0x10
  magic = bytearray(blob)
  magic[0] ^= 0xff
  bound = dev.dec.stream_export_bound()
  inval, cap = _capi.UIS_ERR_INVALID_ARG, _capi.UIS_ERR_CLUSTER_CAP
  return [
      ('bad magic', lambda: _raw_import(dev.dec, 1, bytes(magic)), inval),
      ('truncated by one byte', lambda: _raw_import(dev.dec, 1, blob[:-1]), inval),
      ('one byte short of its size', lambda: _raw_import(dev.dec, 1, blob, len(blob) - 1), inval),
      ('a flipped payload word', lambda: _raw_import(dev.dec, 1, bytes(flipped)), inval),
      ('another model', lambda: _raw_import(dev.dec, 1, other_model_blob), inval),
      ('another beam', lambda: _raw_import(dev.dec, 1, other_beam_blob), inval),
      ('N > max_frames', lambda: _raw_import(dev.dec, 1, long_blob), inval),
      ('K > max_clusters', lambda: _raw_import(dev.dec, 1, big_k_blob), cap),
      ('a target that has received frames', lambda: _raw_import(dev.dec, 0, blob), inval),
      ('utt out of range', lambda: _raw_import(dev.dec, 2, blob), inval),
      ('utt negative', lambda: _raw_import(dev.dec, -1, blob), inval),
      ('export: utt out of range', lambda: _raw_export(dev.dec, 2, bound)[0], inval),
      ('export: capacity below the bound', lambda: _raw_export(dev.dec, 0, bound - 1)[0], inval),
      ('a null blob', lambda: dev.dec._lib.uis_stream_import(dev.dec._handle, 1, None, 64), inval),   # pylint: disable=protected-access
  ]


def _refusal_blobs():
  """Well-formed blobs that a tiny_d16 session of beam 4 and max_frames 12 cannot take."""
  frames = mp.continuation(4).frames
  out = {}
  dev = Dev(golden_util.load_case('toy_d2_depth2')['params'], 1, 4, 16)
  dev.push([golden_util.load_case('toy_d2_depth2')['seqs'][0][:5]])
  out['model'] = dev.dec.stream_export(0)
  dev.close()
  dev = Dev(_params('tiny_d16'), 1, 3, 16)
  dev.push([frames[:5]])
  out['beam'] = dev.dec.stream_export(0)
  dev.close()
  dev = Dev(_params('tiny_d16'), 1, 4, 16)
  dev.push([frames[:13]])
  out['long'] = dev.dec.stream_export(0)
  dev.close()
  return out


def test_refusals_leave_the_session_as_it_was(oracle_lib):
  trace = mp.continuation(4)
  frames = trace.frames
  blobs = _refusal_blobs()
  # a blob of the session's own model with more clusters than its cap of 2: three frames of tiny_d16 at beam 4 reach K = 3
  assert trace.cuts['N3']['K'] == 3
  wide = Dev(_params('tiny_d16'), 1, 4, 16)
  wide.push([frames[:3]])
  big_k = wide.dec.stream_export(0)
  assert _capi.blob_info(big_k)['K'] == 3
  wide.close()
  dev = Dev(_params('tiny_d16'), 2, 4, 12, 2)
  try:
    dev.push([frames[:1], None])
    blob = dev.dec.stream_export(0)
    before = gt.plain(dev.shot())
    assert before[0]['K'] == 1 and before[0]['overflow'] == 0
    for what, call, status in _refusals(dev, blob, blobs['model'], blobs['beam'], blobs['long'], big_k):
      assert call() == status, what
      assert _capi.last_error(dev.dec._lib), what   # pylint: disable=protected-access
      assert gt.plain(dev.shot()) == before, what
    rc, n, raw = _raw_export(dev.dec, 0, dev.dec.stream_export_bound() - 1)
    assert rc == _capi.UIS_ERR_INVALID_ARG and n == -7 and set(raw) == {0x55}      # nothing is written
    dev.dec.stream_prime([None, frames[:2]], [None, np.zeros(2, dtype=np.int32)])
    primed = gt.plain(dev.shot())
    assert _raw_import(dev.dec, 1, blob) == _capi.UIS_ERR_INVALID_ARG              # a target that was primed
    assert 'already received or been primed' in _capi.last_error(dev.dec._lib)     # pylint: disable=protected-access
    assert gt.plain(dev.shot()) == primed
  finally:
    dev.close()
  closed = _capi.Decoder(_params('tiny_d16'))                                      # no session open
  assert _raw_import(closed, 0, blob) == _capi.UIS_ERR_INVALID_ARG and 'no streaming session' in _capi.last_error(closed._lib)   # pylint: disable=protected-access
  assert _raw_export(closed, 0, 1 << 20)[0] == _capi.UIS_ERR_INVALID_ARG
  closed.close()


def test_a_refused_import_costs_a_persistent_session_nothing(oracle_lib, monkeypatch, capfd):
  """Host-decided refusals leave the resident launch on the device: uis_stream_restart's trace line (selecting
  nothing, which does not make it leave either) counts the launches."""
  if not gh._whole_device():   # pylint: disable=protected-access
    pytest.skip('not a whole MI355X')
  monkeypatch.setenv('UIS_RESTART_TRACE', '1')
  monkeypatch.setenv('UIS_PERSIST_IDLE_MS', '2000')
  seqs = golden_util.load_case('tracker_d256')['seqs']
  donor = Dev(_params('tracker_d256'), 1, 4, 40)
  donor.push([seqs[0][:33]])
  long_blob = donor.dec.stream_export(0)
  donor.close()
  dev = Dev(_params('tracker_d256'), 2, 4, 32, 16, _capi.UIS_FLAG_PERSISTENT)
  none = [False, False]
  try:
    dev.push([seqs[0][:5], None])
    dev.dec.stream_restart(none)
    damaged = bytearray(long_blob)
    damaged[100] ^= 1
    for blob, utt in ((long_blob, 1), (bytes(damaged), 1), (long_blob[:-1], 1), (long_blob, 0), (long_blob, 2)):
      assert _raw_import(dev.dec, utt, blob) == _capi.UIS_ERR_INVALID_ARG
    assert _raw_export(dev.dec, 0, 16)[0] == _capi.UIS_ERR_INVALID_ARG
    dev.push([seqs[0][5:10], None])
    dev.dec.stream_restart(none)
    blob = dev.dec.stream_export(0)             # an export makes the launch leave ...
    dev.push([seqs[0][10:11], None])            # ... and the next push starts a new one
    dev.dec.stream_restart(none)
    dev.dec.stream_import(1, blob)
    dev.push([None, seqs[0][10:11]])
    dev.dec.stream_restart(none)
    assert dev.exact(0) == dev.exact(1)
  finally:
    dev.close()
  lines = _lines(capfd.readouterr().err, 'uis_stream_restart')
  assert [int(line['resident_launches']) for line in lines] == [1, 1, 2, 3] and all(line['persistent'] == '1' for line in lines)


def test_dead_utterances_have_nothing_to_move(oracle_lib):
  """tests/hostile.py's overflow case (test_gpu_restart's dead slots): utterances 2 and 3 lose their beam, 5 hits the
  cluster cap, 6 has received nothing -- which is a state like any other."""
  case = hostile.build('overflow', 16, 8, 1, lengths=(12, 9, 15, 8, 14, 11))
  seqs = list(case.seqs) + [np.zeros((0, 16))]
  dev = Dev(case.params, 7, 3, 16, 2)
  try:
    dev.push([s if len(s) else None for s in seqs])
    before = gt.plain(dev.shot())
    assert [c['overflow'] for c in before] == [0, 0, 0, 0, 0, 1, 0] and [c['counts'] for c in before] == [3, 3, 0, 0, 3, 0, 0]
    bound = dev.dec.stream_export_bound()
    want = {2: _capi.UIS_ERR_INVALID_ARG, 3: _capi.UIS_ERR_INVALID_ARG, 5: _capi.UIS_ERR_CLUSTER_CAP}
    for u in range(7):
      rc, n, raw = _raw_export(dev.dec, u, bound)
      assert rc == want.get(u, _capi.UIS_OK), u
      if u in want:
        assert n == -7 and set(raw) == {0x55}, u                  # nothing is written
    assert gt.plain(dev.shot()) == before
    empty = dev.dec.stream_export(6)
    info = _capi.blob_info(empty)
    assert (info['N'], info['committed'], info['live'], info['K'], info['slots']) == (0, 0, 1, 0, 0)
    dev.restart({2})
    dev.dec.stream_import(2, empty)                                # the empty hypothesis arrives: a fresh slot
    dev.push([None, None, seqs[0]] + [None] * 4)
    after = gt.plain(dev.shot())
    assert _exact(after[2]) == _exact(before[0]) and [after[u] for u in (0, 1, 4)] == [before[u] for u in (0, 1, 4)]
  finally:
    dev.close()


# ---- 8. stale memory

@pytest.mark.parametrize('word', WORDS)
def test_no_readout_depends_on_stale_memory(word, oracle_lib, monkeypatch):
  """The targets have held another stream and were restarted (under the knob the restart fills what the stream
  left); scratch and landing block are filled ahead of every call.  Every readout is the reference's."""
  monkeypatch.setenv(KNOB, word)
  monkeypatch.delenv('UIS_NO_ARENA', raising=False)
  for cut in ('N3', 'committed', 'emptied'):
    src, other = _two('tiny_d16', 4, 16, 24)
    try:
      _move(mp.continuation(4), cut, src, other, dirty=True)
    finally:
      src.close()
      other.close()


def test_blob_layout_matches_the_header(oracle_lib):
  """The bytes are what csrc/uis_blob.h says: sections 16-byte aligned, zero pads, the size in the header."""
  trace = mp.continuation(4)
  dev = Dev(_params('tiny_d16'), 1, 4, 16)
  try:
    dev.push([trace.frames[:5]])
    blob = dev.dec.stream_export(0)
    info = _capi.blob_info(blob)
    assert info['bytes'] == len(blob) and len(blob) % 16 == 0 and len(blob) <= dev.dec.stream_export_bound()
    magic, fmt, numerics, look = struct.unpack_from('<4I', blob, 0)
    assert (magic, fmt, look) == (_capi.BLOB_MAGIC, 1, 1) and numerics == dev.dec._lib.uis_numerics_version()   # pylint: disable=protected-access
    assert info['N'] == 5 and info['live'] == trace.cuts['N5']['live'] and info['K'] == trace.cuts['N5']['K']
    checksum, end = struct.unpack_from('<QQ', blob, len(blob) - 16)
    assert end == 0x444e454253495555 and checksum != 0
    records = len(blob) - 16 - 16 * ((5 * 4 * 4 + 15) // 16)        # N * B words, padded to 16 bytes
    labels = [int(v) & 0xffff for v in np.frombuffer(blob, dtype='<u4', count=20, offset=records)]
    assert labels[16] == dev.col(0)['labels'][4]                     # rank 0's record of the last step: the best label
  finally:
    dev.close()
