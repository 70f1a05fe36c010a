"""Session restarts (uis_stream_restart): end one utterance of a live session and reuse its slot in place.

Every comparison is exact: integer labels, float32 bit patterns.  The reference is a slot's stream decoded on its
own -- oracle.decode for labels and score, nbest_ref.replay / commit_ref for the beam and for commits -- and every
slot is held to it at every push, so a slot that is never restarted reads as in a session without restarts.
  1. a recycled slot is a fresh session (all session paths)      5. other model shapes
  2. neighbours are untouched                                    6. prime after restart
  3. with commits, the endless session                           7. refusals
  4. dead slots come back                                        8. stale memory      9. the Python layer
"""

import ctypes
import functools
import os

import numpy as np
import pytest

import commit_ref
import golden_util
import hostile
import nbest_ref
import primed_ref
import test_gpu_hostile as gh
import uisrnn_amd
from oracle import oracle
from uisrnn_amd import _capi
from uisrnn_amd import synth

pytestmark = pytest.mark.gpu

WORDS = ('ffffffff', '7f7f7f7f', '80000000')
KNOB = 'UIS_POISON_WORKSPACE'
_i32p = ctypes.POINTER(ctypes.c_int32)
PER_UTT = ('labels', 'scores', 'beam', 'overflow', 'rows', 'nb_scores', 'counts', 'stable')


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(name):
  oracle.lib()
  return golden_util.load_case(name)


@functools.lru_cache(maxsize=None)
def _replays(name, beam):
  case = _case(name)
  return [nbest_ref.replay(case['params'], s, beam) for s in case['seqs']]


@functools.lru_cache(maxsize=None)
def _model(name):
  return primed_ref.Model(_case(name)['params'])


@functools.lru_cache(maxsize=None)
def _offline(name, beam, idx, upto):
  """(labels, score bits) of the offline decode of the first `upto` frames of the case's sequence idx."""
  case = _case(name)
  out = oracle.decode(case['params'], [case['seqs'][idx][:upto]], beam, 1, 1)
  return out['labels'][0].tolist(), int(_bits(out['scores'])[0])


class _Session:
  """An open session of a Decoder plus the labels it has committed (what OnlineSession keeps)."""

  def __init__(self, dec, n_utt, beam):
    self.dec, self.n_utt, self.beam = dec, n_utt, beam
    self.final = [[] for _ in range(n_utt)]

  def snapshot(self):
    """Every readout, for the whole stream, in plain Python values."""
    dec = self.dec
    lab, scores, overflow, status = dec.stream_labels()
    info = np.empty((self.n_utt, self.beam), dtype=np.float32)
    dec._check(dec._lib.uis_last_decode_info(dec._handle, None, info.ctypes.data_as(_capi._fp)), 'info')  # pylint: disable=protected-access
    nb = dec.stream_nbest(self.beam)
    counts = nb['counts'].tolist()
    return {
        'labels': [self.final[u] + lab[u].tolist() for u in range(self.n_utt)],
        'scores': _bits(scores).tolist(), 'beam': _bits(info).tolist(), 'overflow': overflow.tolist(),
        'status': (status, nb['status']),
        'rows': [[self.final[u] + row.tolist() for row in nb['labels'][u][:counts[u]]] for u in range(self.n_utt)],
        'nb_scores': _bits(nb['scores']).tolist(), 'counts': counts,
        'stable': [len(self.final[u]) + int(nb['stable'][u]) for u in range(self.n_utt)],
    }

  def commit(self, horizon=None):
    hz = None if horizon is None else [horizon] * self.n_utt if isinstance(horizon, int) else horizon
    have = self.dec.stream_received()
    out, dropped = self.dec.stream_commit(hz)
    for u in range(self.n_utt):
      self.final[u].extend(out[u].tolist())
    assert self.dec.stream_received().tolist() == (have - np.array([len(o) for o in out])).tolist()
    assert self.dec.stream_committed().tolist() == [len(f) for f in self.final]
    return [o.tolist() for o in out], dropped.tolist()

  def restart(self, which):
    """Restart the slots in `which`.  Returns ({slot: dict(labels of the whole stream, window, score bits, overflow)},
    status); checks the host's bookkeeping on the way."""
    have, done = self.dec.stream_received(), self.dec.stream_committed()
    labels, scores, overflow, status = self.dec.stream_restart([u in which for u in range(self.n_utt)])
    got = {}
    for u in range(self.n_utt):
      if u in which:
        assert len(labels[u]) == have[u], u
        got[u] = {'labels': self.final[u] + labels[u].tolist(), 'window': labels[u].tolist(),
                  'score': int(_bits(scores[u:u + 1])[0]), 'overflow': int(overflow[u])}
        self.final[u] = []
        have[u] = done[u] = 0
      else:
        assert len(labels[u]) == 0 and overflow[u] == 0 and np.isnan(scores[u]), u   # (entries not selected are not written)
    assert self.dec.stream_received().tolist() == have.tolist()
    assert self.dec.stream_committed().tolist() == done.tolist()
    return got, status


def _col(shot, u):
  return {k: shot[k][u] for k in PER_UTT}


def _fresh(beam):
  """What every readout says about an utterance that has received nothing."""
  inf = _bits(np.full(beam, np.inf)).tolist()
  return {'labels': [], 'scores': int(_bits(np.zeros(1))[0]), 'beam': inf, 'overflow': 0, 'rows': [], 'nb_scores': inf,
          'counts': 0, 'stable': 0}


def _want(labels, rows, scores, stable, beam):
  """A reference's readouts of one utterance as a snapshot column."""
  if not rows and not labels:
    return _fresh(beam)
  padded = _bits(primed_ref.padded_beam(scores, beam)).tolist()
  return {'labels': labels, 'scores': padded[0], 'beam': padded, 'overflow': 0, 'rows': rows, 'nb_scores': padded,
          'counts': len(rows), 'stable': stable}


class _ReplayStream:
  """A stream that never commits, read off the oracle's replay of its sequence."""

  def __init__(self, name, beam, idx):
    self.rep, self.beam, self.received = _replays(name, beam)[idx], beam, 0

  def push(self, part):
    self.received += len(part)

  def want(self):
    rows, scores = nbest_ref.nbest(self.rep, upto=self.received)
    return _want(rows[0].tolist() if len(rows) else [], rows.tolist(), scores, nbest_ref.common_prefix(rows), self.beam)

  def commit(self, horizon):
    raise AssertionError('a replay does not commit')

  def width(self, upto):
    return self.rep.parents[upto - 1].size if upto else 0


class _CommitStream:
  """A stream that commits: commit_ref.Session from scratch, driven in lock-step with the device."""

  def __init__(self, name, beam, idx):
    del idx
    self.ref, self.beam = commit_ref.Session(_model(name), beam), beam

  @property
  def received(self):
    return self.ref.received

  def push(self, part):
    self.ref.push(part)

  def want(self):
    ref = self.ref
    return _want(ref.labels(), [ref.final + r.tolist() for r in ref.rows()], ref.scores(), ref.committed + ref.stable(), self.beam)

  def commit(self, horizon):
    return self.ref.commit(horizon)


def _drive(dec, name, beam, flags, plan, chunk=7, window=None, horizon=None, empty=None, log=None, slots=None, stop=None):
  """One session of all the case's utterances pushed in chunks of `chunk`; after push k the slots plan[k] restart and
  go on with the case's NEXT sequence.  Every slot is compared with its reference after every push, before and
  after every commit and restart.  horizon: commit(horizon) after every push; empty = (push, slot): that slot
  commits with horizon 0 there instead (its window empties if it holds an even number of frames).  slots: the
  sequences the session starts with (default: all of the case's, one slot each); stop: the last push (default:
  when every stream has ended).
  Returns what the restarts saw: a list of dict(slot, seq, upto, have, committed, full, labels)."""
  what = (name, beam, flags, chunk, horizon)
  case = _case(name)
  seqs = case['seqs']
  slots = list(range(len(seqs))) if slots is None else list(slots)
  n = len(slots)
  make = (lambda idx: _ReplayStream(name, beam, idx)) if horizon is None else (lambda idx: _CommitStream(name, beam, idx))
  dec.stream_begin(n, beam, window or max(len(s) for s in seqs), flags=flags)
  seen = []
  try:
    session = _Session(dec, n, beam)
    stream, pos = list(slots), [0] * n
    refs = [make(idx) for idx in stream]
    k = 0
    while (k <= max(plan) or any(pos[u] < len(seqs[stream[u]]) for u in range(n))) if stop is None else k <= stop:
      parts = [seqs[stream[u]][pos[u]:pos[u] + chunk] for u in range(n)]
      dec.stream_push([p if len(p) else None for p in parts])
      for u in range(n):
        refs[u].push(parts[u])
        pos[u] += len(parts[u])
      shot = session.snapshot()
      if log is not None:
        log.append(shot)
      for u in range(n):
        assert _col(shot, u) == refs[u].want(), what + (k, u)
      if horizon is not None:
        hz = [0 if empty == (k, u) else horizon for u in range(n)]
        got = session.commit(hz)
        for u in range(n):
          assert (got[0][u], got[1][u]) == refs[u].commit(hz[u]), what + (k, u)
        shot = session.snapshot()
        for u in range(n):
          assert _col(shot, u) == refs[u].want(), what + ('committed', k, u)
      if k in plan:
        which = set(plan[k])
        done = dec.stream_committed().tolist()
        have = dec.stream_received().tolist()
        got, status = session.restart(which)
        assert status == _capi.UIS_OK, what + (k,)
        after = session.snapshot()
        if log is not None:
          log.extend([got, after])
        for u in range(n):
          if u not in which:   # 2. the neighbours: every readout as before
            assert _col(after, u) == _col(shot, u), what + ('neighbour', k, u)
            continue
          assert got[u]['labels'] == shot['labels'][u] and got[u]['score'] == shot['scores'][u], what + ('handed out', k, u)
          assert got[u]['overflow'] == 0, what + (k, u)
          assert _col(after, u) == _fresh(beam), what + ('fresh', k, u)
          seen.append({'slot': u, 'seq': stream[u], 'upto': pos[u], 'have': have[u], 'committed': done[u],
                       'full': shot['counts'][u] == beam, 'labels': got[u]['labels'], 'score': got[u]['score']})
          stream[u], pos[u] = (stream[u] + 1) % len(seqs), 0
          refs[u] = make(stream[u])
      k += 1
    assert dec.stream_labels()[3] == _capi.UIS_OK
    return seen, [(stream[u], pos[u]) for u in range(n)], session.snapshot()
  finally:
    dec.stream_end()


# ---- 1. a recycled slot is a fresh session / 2. neighbours are untouched

def _plan(name):
  """A non-contiguous subset after the first push, all after the third, none after the fourth, one slot later
  (tracker_d256: the slot that is 56 frames into the case's second sequence, the only one that opens a third cluster)."""
  if name == 'tracker_d256':
    return {0: (0, 2), 2: (0, 1, 2), 3: (), 10: (2,)}
  return {0: (0, 2, 5), 2: tuple(range(6)), 3: (), 5: (1,)}


def _fresh_slot_case(dec, name, beam, flags, log=None):
  seen, last, final = _drive(dec, name, beam, flags, _plan(name), log=log)
  n = len(_case(name)['seqs'])
  # the labels and scores handed out, and the last streams' at the end, are the offline decode's
  for r in seen:
    assert (r['labels'], r['score']) == _offline(name, beam, r['seq'], r['upto']), (name, beam, flags, r['slot'], r['seq'])
  for u, (idx, upto) in enumerate(last):
    assert (final['labels'][u], final['scores'][u]) == _offline(name, beam, idx, upto), (name, beam, flags, u)
    assert upto == len(_case(name)['seqs'][idx])
  # the reference's conditions: odd and even windows, three clusters, a full beam replaced by a narrow one
  assert any(r['have'] % 2 == 1 for r in seen) and any(r['have'] % 2 == 0 and r['have'] > 0 for r in seen)
  assert any(len(set(r['labels'])) >= 3 for r in seen), [len(set(r['labels'])) for r in seen]
  reps = _replays(name, beam)
  assert any(r['full'] and reps[(r['seq'] + 1) % n].parents[0].size < beam for r in seen)
  return seen


def _paths(name):
  if name == 'tracker_d256':
    return (('default', 0), ('stepwise', _capi.UIS_FLAG_STEPWISE), ('resident', _capi.UIS_FLAG_RESIDENT))
  return (('default', 0), ('stepwise', _capi.UIS_FLAG_STEPWISE))


@pytest.mark.parametrize('name', ['tracker_d256', 'tiny_d16'])
@pytest.mark.parametrize('beam', [10, 4, 3])
def test_a_recycled_slot_is_a_fresh_session(name, beam, oracle_lib):
  dec = _capi.Decoder(_case(name)['params'])
  for _, flags in _paths(name):
    _fresh_slot_case(dec, name, beam, flags)
  dec.close()


def _trace_lines(err):
  return [dict(zip(line.split()[1::2], line.split()[2::2])) for line in err.splitlines() if line.startswith('uis_stream_restart:')]


@pytest.mark.parametrize('beam', [10, 4, 3])
def test_a_persistent_session_stays_persistent(beam, oracle_lib, monkeypatch, capfd):
  if not gh._whole_device():   # pylint: disable=protected-access
    pytest.skip('not a whole MI355X')
  monkeypatch.setenv('UIS_RESTART_TRACE', '1')
  name = 'tracker_d256'
  dec = _capi.Decoder(_case(name)['params'])
  _fresh_slot_case(dec, name, beam, _capi.UIS_FLAG_PERSISTENT)
  dec.close()
  lines = _trace_lines(capfd.readouterr().err)
  assert len(lines) == len(_plan(name)) and all(line['persistent'] == '1' for line in lines), lines
  assert [line['selected'] for line in lines] == ['2', '3', '0', '1']
  launches = [int(line['resident_launches']) for line in lines]
  assert launches == sorted(launches) and launches[0] >= 1


@pytest.mark.parametrize('name,beam', [('tracker_d256', 4), ('tiny_d16', 10)])
def test_a_slot_that_is_never_restarted_reads_as_in_a_session_without_restarts(name, beam, oracle_lib):
  n = len(_case(name)['seqs'])
  subset = (0, 2) if n == 3 else (0, 2, 5)
  dec = _capi.Decoder(_case(name)['params'])
  with_restarts, without = [], []
  _drive(dec, name, beam, 0, {0: subset, 2: subset, 3: ()}, log=with_restarts)
  _drive(dec, name, beam, 0, {0: ()}, log=without)
  dec.close()
  a, b = _per_push(with_restarts), _per_push(without)
  assert len(a) >= len(b) >= -(-max(len(s) for s in _case(name)['seqs']) // 7)
  for k, quiet in enumerate(b):
    for u in range(n):
      if u not in subset:
        assert _col(a[k], u) == _col(quiet, u), (name, k, u)


def _per_push(log):
  """The snapshots taken right after a push: a restart appends (its result, the snapshot after it) behind one."""
  out, skip = [], False
  for entry in log:
    if skip:
      skip = False
      continue
    if 'status' in entry:
      out.append(entry)
    else:          # a restart's result: the next entry is the snapshot taken after it
      skip = True
  return out


# ---- 3. with commits

COMMIT_CASES = {
    # name: (beam, chunk, window, plan, (push, slot) whose commit uses horizon 0, the slots' first sequences, last push).
    # tracker_d256 runs two slots for four pushes of 5 frames: tests/commit_ref.py's beam search in Python takes a
    # quarter of a second per frame at this size, and everything the case is for has happened by then
    'tiny_d16': (4, 7, 16, {1: (0,), 2: (1, 3), 3: (0, 2, 4)}, (1, 0), None, None),
    'tracker_d256': (10, 5, 16, {1: (1,), 2: (0,)}, (1, 1), (1, 2), 3),
}


def _commit_case(dec, name, log=None):
  beam, chunk, window, plan, empty, slots, stop = COMMIT_CASES[name]
  assert window < max(len(s) for s in _case(name)['seqs'])
  seen, _, _ = _drive(dec, name, beam, 0, plan, chunk=chunk, window=window, horizon=8, empty=empty, log=log, slots=slots, stop=stop)
  # the reference's conditions: every restarted slot named in the plan's first steps had committed; one window was
  # emptied by the commit just before; odd and even windows behind an (always even) commit
  emptied = [r for r in seen if r['have'] == 0 and r['committed'] > 0]
  assert emptied and emptied[0]['slot'] == empty[1], seen
  busy = [r for r in seen if r['committed'] > 0 and r['have'] > 0]
  assert any(r['have'] % 2 == 1 for r in busy), [(r['have'], r['committed']) for r in seen]
  if name == 'tiny_d16':
    assert any(r['have'] % 2 == 0 for r in busy), [(r['have'], r['committed']) for r in seen]
  assert all(r['committed'] % 2 == 0 for r in seen)
  return seen


@pytest.mark.parametrize('name', sorted(COMMIT_CASES))
def test_restarts_in_a_session_that_commits(name, oracle_lib):
  dec = _capi.Decoder(_case(name)['params'])
  _commit_case(dec, name)
  dec.close()


LONG_FRAMES, LONG_WINDOW, LONG_HORIZON, LONG_CHUNK = 200, 64, 32, 5


@functools.lru_cache(maxsize=None)
def _long_seq(seed):
  return np.asarray(synth.make_utterance(seed, LONG_FRAMES, 16)[0], dtype=np.float64)


def _online(name, beam, max_clusters=None):
  params = _case(name)['params'] if isinstance(name, str) else name
  model_args, _, args = uisrnn_amd.parse_arguments(
      ['--observation_dim', str(int(params['observation_dim'])), '--rnn_hidden_size', str(int(params['rnn_hidden_size']))])
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params)
  args.beam_size, args.look_ahead, args.test_iteration = beam, 1, 1
  if max_clusters:
    args.max_clusters = max_clusters
  return model, args


def test_an_endless_session_restarts_in_mid_stream(oracle_lib):
  """Two long streams through one slot of a session that commits by itself: each equals its own endless session,
  push by push.  (A push that does not fit commits EVERY utterance, so a neighbour that made the session commit at
  other pushes would change what the horizon decides; the neighbour here stays shorter than the horizon, where a
  commit only moves its window.)"""
  beam, cut, short = 4, 120, 30
  first, second, other = _long_seq(4242), _long_seq(777), _long_seq(99)[:short]
  model, args = _online('tiny_d16', beam)
  solo = {}
  for key, seq in (('first', first[:cut]), ('second', second)):
    with model.online(1, args, LONG_WINDOW, horizon=LONG_HORIZON) as session:
      solo[key] = []
      for lo in range(0, len(seq), LONG_CHUNK):
        session.push([seq[lo:lo + LONG_CHUNK]])
        solo[key].append((session.committed[0], session.labels()[0] if lo % 40 == 0 or lo + LONG_CHUNK >= len(seq) else None))
      solo[key + '/end'] = (session.labels()[0], session.nbest(1)[0][1][0])
  assert max(c for c, _ in solo['first']) > 0 and max(c for c, _ in solo['second']) > LONG_WINDOW
  beside = model.predict(other, args)
  with model.online(2, args, LONG_WINDOW, horizon=LONG_HORIZON) as session:
    def feed(seq, key, o0):
      for k, lo in enumerate(range(0, len(seq), LONG_CHUNK)):
        o = o0 + lo
        session.push([seq[lo:lo + LONG_CHUNK], other[o:o + LONG_CHUNK] if o < short else None])
        assert session.committed[0] == solo[key][k][0], (key, lo)
        if solo[key][k][1] is not None:
          assert session.labels()[0] == solo[key][k][1], (key, lo)
    feed(first[:cut], 'first', 0)
    assert session.committed[0] > 0 and session.labels()[1] == beside
    neighbour = session.committed[1]
    out = session.restart([0])
    assert out[1] is None and out[0][0] == solo['first/end'][0]
    assert _bits(out[0][1]).tolist() == _bits(solo['first/end'][1]).tolist()
    assert session.committed == [0, neighbour] and session.labels() == [[], beside]
    assert session.stable_frames()[0] == 0
    feed(second, 'second', cut)
    assert session.labels() == [solo['second/end'][0], beside]
    assert _bits(session.nbest(1)[0][1][0]).tolist() == _bits(solo['second/end'][1]).tolist()


# ---- 4. dead slots come back

def _dead_case():
  case = hostile.build('overflow', 16, 8, 1, lengths=(12, 9, 15, 8, 14, 11))
  return case, list(case.seqs) + [np.zeros((0, 16))]


def test_dead_slots_come_back(oracle_lib):
  """test_gpu_commit's excluded utterances: 2 and 3 lose their beam, 5 hits the cluster cap, 6 is empty."""
  beam, cap = 3, 2
  case, seqs = _dead_case()
  dead = (2, 3, 5, 6)
  dec = _capi.Decoder(case.params)
  dec.stream_begin(7, beam, 16, max_clusters=cap)
  try:
    session = _Session(dec, 7, beam)
    dec.stream_push([s if len(s) else None for s in seqs])
    first = session.snapshot()
    assert first['overflow'] == [0, 0, 0, 0, 0, 1, 0] and first['counts'] == [3, 3, 0, 0, 3, 0, 0]
    lab, scores, _, status = dec.stream_labels()
    assert status == _capi.UIS_ERR_CLUSTER_CAP
    got, status = session.restart(set(dead))
    assert status == _capi.UIS_ERR_CLUSTER_CAP
    assert [got[u]['overflow'] for u in dead] == [0, 0, 1, 0]
    for u in dead:
      assert got[u]['window'] == lab[u].tolist() and len(lab[u]) == len(seqs[u]), u
      assert got[u]['score'] == int(_bits(scores)[u]), u
    assert all(v == -1 for u in (2, 3) for v in got[u]['window'])
    after = session.snapshot()
    assert after['status'] == (_capi.UIS_OK, _capi.UIS_OK)
    for u in range(7):
      assert _col(after, u) == (_fresh(beam) if u in dead else _col(first, u)), u
    dec.stream_push([seqs[0] if u in dead else None for u in range(7)])
    again = session.snapshot()
    assert again['status'] == (_capi.UIS_OK, _capi.UIS_OK)
    for u in range(7):
      assert _col(again, u) == _col(first, 0 if u in dead else u), u
    assert again['overflow'] == [0] * 7
  finally:
    dec.stream_end()
  dec.close()


# ---- 5. other model shapes

@pytest.mark.parametrize('name,beam,chunk,at', [('tracker_d64_h300', 2, 7, 1), ('toy_d2_depth2', 3, 1, 12)])
def test_a_restart_on_other_model_shapes(name, beam, chunk, at, oracle_lib):
  dec = _capi.Decoder(_case(name)['params'])
  for flags in (0, _capi.UIS_FLAG_STEPWISE):
    seen, last, final = _drive(dec, name, beam, flags, {at: (0, 2)}, chunk=chunk)
    assert len(seen) == 2 and all(r['have'] == (at + 1) * chunk for r in seen)
    for r in seen:
      assert (r['labels'], r['score']) == _offline(name, beam, r['seq'], r['upto']), (name, flags, r['slot'])
    for u, (idx, upto) in enumerate(last):
      assert (final['labels'][u], final['scores'][u]) == _offline(name, beam, idx, upto), (name, flags, u)
  dec.close()


# ---- 6. prime after restart

def test_a_restarted_slot_accepts_a_prefix(oracle_lib):
  name, beam, plen = 'tiny_d16', 4, 6
  case = _case(name)
  seqs = case['seqs']
  prefix = oracle.decode(case['params'], [seqs[3]], 1, 1, 1)['labels'][0][:plen].astype(np.int32)
  want = primed_ref.primed_decode(case['params'], seqs[3], prefix, beam)
  dec = _capi.Decoder(case['params'])
  dec.stream_begin(2, beam, 32)
  try:
    session = _Session(dec, 2, beam)
    dec.stream_push([seqs[0][:14], seqs[1][:5]])
    session.commit(8)
    assert dec.stream_committed()[0] > 0
    have1 = int(dec.stream_received()[1])
    for u in (0, 1):   # both have received frames: neither can be primed
      with pytest.raises(_capi.HipLibraryError, match='already received') as err:
        dec.stream_prime([seqs[3][:plen] if v == u else None for v in (0, 1)], [prefix if v == u else None for v in (0, 1)])
      assert err.value.status == _capi.UIS_ERR_INVALID_ARG
    before = session.snapshot()
    session.restart({0})
    primed = dec.stream_prime([seqs[3][:plen], None], [prefix, None])
    assert _bits(primed)[0] == _bits(want['prefix_score']) and dec.stream_received().tolist() == [plen, have1]
    with pytest.raises(_capi.HipLibraryError, match='already received') as err:   # the neighbour still refuses
      dec.stream_prime([None, seqs[3][:plen]], [None, prefix])
    assert err.value.status == _capi.UIS_ERR_INVALID_ARG
    dec.stream_push([seqs[3][plen:], None])
    shot = session.snapshot()
    rows = want['labels'].tolist()
    assert _col(shot, 0) == _want(rows[0], rows, want['scores'], nbest_ref.common_prefix(want['labels']), beam)
    assert _col(shot, 1) == _col(before, 1)
  finally:
    dec.stream_end()
  dec.close()


# ---- 7. refusals

def _raw_restart(dec, which, labels, capacity, counts, scores=None, overflow=None):
  ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)   # pylint: disable=unnecessary-lambda-assignment
  return dec._lib.uis_stream_restart(dec._handle, ptr(which, _i32p), ptr(labels, _i32p), capacity, ptr(counts, _i32p),   # pylint: disable=protected-access
                                     ptr(scores, _capi._fp), ptr(overflow, _i32p))   # pylint: disable=protected-access


def test_refusals_leave_the_session_as_it_was(oracle_lib):
  name, beam = 'tiny_d16', 4
  case = _case(name)
  seqs = case['seqs'][:4]
  dec = _capi.Decoder(case['params'])
  which = np.array([1, 0, 1, 0], dtype=np.int32)
  counts = np.full(4, -7, dtype=np.int32)
  labels = np.full(64, -7, dtype=np.int32)
  scores = np.full(4, -7.0, dtype=np.float32)
  overflow = np.full(4, -7, dtype=np.int32)
  untouched = lambda: (counts == -7).all() and (labels == -7).all() and (scores == -7.0).all() and (overflow == -7).all()   # pylint: disable=unnecessary-lambda-assignment
  assert _raw_restart(dec, which, labels, 64, counts, scores, overflow) == _capi.UIS_ERR_INVALID_ARG      # no session open
  assert untouched()
  dec.stream_begin(4, beam, 32)
  try:
    session = _Session(dec, 4, beam)
    dec.stream_push([s[:12] for s in seqs])
    session.commit(8)
    before = session.snapshot()
    have, done = dec.stream_received().tolist(), dec.stream_committed().tolist()
    assert sum(done) > 0
    due = have[0] + have[2]
    for args in ((None, labels, 64, counts), (which, labels, 64, None), (which, labels, due - 1, counts), (which, None, 64, counts)):
      assert _raw_restart(dec, *args, scores=scores, overflow=overflow) == _capi.UIS_ERR_INVALID_ARG, args[2]
      assert untouched()
      assert dec.stream_received().tolist() == have and dec.stream_committed().tolist() == done
      assert session.snapshot() == before
    # selecting nothing
    assert _raw_restart(dec, np.zeros(4, dtype=np.int32), None, 0, counts, scores, overflow) == _capi.UIS_OK
    assert counts.tolist() == [0] * 4 and (scores == -7.0).all() and (overflow == -7).all()
    assert session.snapshot() == before
    # exactly the capacity due; entries of utterances not selected are not written
    counts[:] = -7
    assert _raw_restart(dec, which, labels, due, counts, scores, overflow) == _capi.UIS_OK
    assert counts.tolist() == [have[0], 0, have[2], 0] and (labels[due:] == -7).all()
    assert labels[:due].tolist() == before['labels'][0][done[0]:] + before['labels'][2][done[2]:]
    assert _bits(scores)[[0, 2]].tolist() == [before['scores'][0], before['scores'][2]] and scores[1] == scores[3] == -7.0
    assert overflow.tolist() == [0, -7, 0, -7]
    assert dec.stream_committed().tolist() == [0, done[1], 0, done[3]]
  finally:
    dec.stream_end()
  dec.close()


def test_selecting_nothing_leaves_the_resident_launch_alone(oracle_lib, monkeypatch, capfd):
  if not gh._whole_device():   # pylint: disable=protected-access
    pytest.skip('not a whole MI355X')
  monkeypatch.setenv('UIS_RESTART_TRACE', '1')
  monkeypatch.setenv('UIS_PERSIST_IDLE_MS', '2000')
  case = _case('tracker_d256')
  seqs = case['seqs']
  dec = _capi.Decoder(case['params'])
  dec.stream_begin(3, 4, 60, flags=_capi.UIS_FLAG_PERSISTENT)
  try:
    none = [False] * 3
    for lo in range(3):
      dec.stream_push([s[lo:lo + 1] for s in seqs])
      assert dec.stream_restart(none)[3] == _capi.UIS_OK
    dec.stream_restart([True, False, False])
    dec.stream_push([s[3:4] for s in seqs])
    dec.stream_restart(none)
  finally:
    dec.stream_end()
  dec.close()
  lines = _trace_lines(capfd.readouterr().err)
  assert [line['selected'] for line in lines] == ['0', '0', '0', '1', '0']
  assert all(line['persistent'] == '1' for line in lines)
  assert [int(line['resident_launches']) for line in lines] == [1, 1, 1, 1, 2]


# ---- 8. stale memory

@functools.lru_cache(maxsize=None)
def _plain_runs():
  """Cases 1 (tiny_d16) and 3 (the emptied window) without the knob: every snapshot and everything handed out."""
  assert KNOB not in os.environ
  return _stale_runs()


def _stale_runs():
  dec = _capi.Decoder(_case('tiny_d16')['params'])
  logs = []
  for flags in (0, _capi.UIS_FLAG_STEPWISE):
    logs.append([])
    _fresh_slot_case(dec, 'tiny_d16', 4, flags, log=logs[-1])
  logs.append([])
  _commit_case(dec, 'tiny_d16', log=logs[-1])
  dec.close()
  return logs


@pytest.mark.parametrize('word', WORDS)
def test_no_output_depends_on_stale_memory(word, oracle_lib, monkeypatch):
  monkeypatch.delenv(KNOB, raising=False)
  monkeypatch.delenv('UIS_NO_ARENA', raising=False)
  plain = _plain_runs()
  monkeypatch.setenv(KNOB, word)
  assert _stale_runs() == plain


# ---- 9. the Python layer

def test_a_stream_pool_recycles_its_slots(oracle_lib):
  """Three slots, seven sequences queued (tiny_d16's six and a synthetic one): each slot takes the next when its
  stream ends; every finish is predict's answer."""
  name, beam = 'tiny_d16', 4
  queue = [np.asarray(s, dtype=np.float64) for s in _case(name)['seqs']]
  queue.append(np.asarray(synth.make_utterance(5, 17, 16)[0], dtype=np.float64))
  model, args = _online(name, beam)
  want = model.predict(queue, args)
  done, waiting, pos = {}, list(range(len(queue))), {}
  with model.online_pool(3, args, max_frames=32) as pool:
    while waiting or pos:
      while waiting and len(pos) < 3:
        pool.open(waiting[0])
        pos[waiting.pop(0)] = 0
      if len(pos) == 3 and waiting:
        with pytest.raises(RuntimeError, match='no free slot'):
          pool.open(waiting[0])
      with pytest.raises(KeyError):
        pool.open(next(iter(pos)))
      pool.push({key: queue[key][at:at + 5] for key, at in pos.items()})
      for key in list(pos):
        pos[key] += 5
        if pos[key] >= len(queue[key]):
          assert pool.labels(key) == want[key], key
          done[key] = pool.finish(key)
          del pos[key]
  assert [done[key][0] for key in range(len(queue))] == want
  scores = model.predict_nbest(queue, args, 1)
  assert [_bits(done[key][1]).tolist() for key in range(len(queue))] == [_bits(s[1][0]).tolist() for s in scores]


def test_online_session_restart(oracle_lib):
  beam, cap = 3, 2
  case, seqs = _dead_case()
  model, args = _online(case.params, beam, max_clusters=cap)
  seqs = [np.asarray(s, dtype=np.float64) for s in seqs]
  with model.online(7, args, max_frames=16) as session:
    session.push([s if len(s) else None for s in seqs])
    with pytest.raises(RuntimeError, match='max_clusters'):
      session.labels()
    for bad in ([7], [-1], [0, 0]):
      with pytest.raises(ValueError):
        session.restart(bad)
    out = session.restart([2, 5, 6])
    assert [o is None for o in out] == [True, True, False, True, True, False, False]
    assert out[2][0] is None and out[5][0] is None and np.isinf(out[2][1])     # an emptied beam, the cluster cap
    assert out[6] == ([], 0.0)
    labels = session.labels()                                                   # nobody is over the cap any more
    ref = oracle.decode(case.params, case.seqs, beam, 1, 1)
    assert [labels[u] for u in (0, 1, 4)] == [ref['labels'][u].tolist() for u in (0, 1, 4)]
    session.push([None, None, seqs[0], None, None, seqs[1], seqs[4]])
    labels = session.labels()
    assert [labels[u] for u in (2, 5, 6)] == [ref['labels'][u].tolist() for u in (0, 1, 4)]
    assert session.restart([5])[5] == (ref['labels'][1].tolist(), float(ref['scores'][1]))
