"""Session commits (uis_stream_commit): endless online decoding in a fixed window.

Every comparison is exact: integer labels, float32 bit patterns.
  1. transparency  without a horizon a session that commits after every push answers every readout -- labels, the
                   final beam's scores, all n-best rows, the stable prefix -- as the session that never commits, on
                   every session path; its committed counts are commit_ref's
  2. horizon       the cut / prune / commit rule against tests/commit_ref.py, and on the device alone: after
                   commit(horizon=0) a session IS a session primed with its labels
  3. longer than the window   400 frames through a window of 16
  4. the edges of k_commit_prune and k_commit_move
  5. refusals leave the session as it was; UIS_POISON_WORKSPACE
"""

import ctypes
import functools

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
MOVE_TILE_WORDS = 1024   # UIS_COMMIT_TILE_WORDS of uisrnn_amd/csrc/uis_commit.hip: k_commit_move's tile
_i32p = ctypes.POINTER(ctypes.c_int32)


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


def _chunks(seqs, lo, chunk):
  return [s[lo:lo + chunk] if lo < len(s) else None for s in seqs]


def _moves(history):
  """(commits that moved a retained part longer than the committed one, ... a shorter one)."""
  done = [h for h in history if h.committed]
  return (sum(1 for h in done if h.have - h.committed > h.committed), sum(1 for h in done if h.have - h.committed < h.committed))


def _not_vacuous(sessions, lengths, what):
  """The issue's condition on the REFERENCE: an utterance commits at least half of its frames, a commit moves a
  retained part longer than the committed one (source and destination overlap) and one a shorter part."""
  assert any(2 * s.committed >= n for s, n in zip(sessions, lengths)), what
  longer, shorter = (sum(x) for x in zip(*[_moves(s.history) for s in sessions]))
  assert longer >= 1 and shorter >= 1, (what, longer, shorter)


# ---- 1. transparency

def _transparent(dec, params, seqs, reps, beam, chunk, flags, what, max_clusters=0):
  del params
  n_utt, longest = len(seqs), max(len(s) for s in seqs)
  refs = [commit_ref.ReplaySession(r) for r in reps]
  shots = {}
  for commits in (False, True):
    dec.stream_begin(n_utt, beam, longest, max_clusters=max_clusters, flags=flags)
    try:
      session = _Session(dec, n_utt, beam)
      shots[commits] = []
      for lo in range(0, longest, chunk):
        dec.stream_push(_chunks(seqs, lo, chunk))
        shot = session.snapshot()
        shots[commits].append(shot)
        if not commits:
          assert dec.stream_committed().tolist() == [0] * n_utt
          continue
        out, dropped = session.commit()
        for u, ref in enumerate(refs):
          ref.push(max(0, min(chunk, len(seqs[u]) - lo)))
          assert out[u] == ref.commit()[0], (what, lo, u)
        assert dropped == [0] * n_utt, (what, lo)
        assert [len(f) for f in session.final] == [r.committed for r in refs], (what, lo)
        # the window moved, the answers did not
        lab = dec.stream_labels()[0]
        assert [session.final[u] + lab[u].tolist() for u in range(n_utt)] == shot['labels'], (what, lo)
        assert session.snapshot() == shot, (what, lo)   # (also where the commit emptied a window: its one hypothesis stays)
    finally:
      dec.stream_end()
  assert shots[True] == shots[False], what
  for u, ref in enumerate(refs):   # (and the answers are the replay's)
    rows = nbest_ref.nbest(reps[u])[0]
    assert shots[True][-1]['rows'][u] == rows.tolist(), (what, u)
    assert ref.final == rows[0][:ref.committed].tolist()
  _not_vacuous(refs, [len(s) for s in seqs], what)


def _paths(name):
  if name == 'tracker_d256':
    return (('default', 0), ('stepwise', _capi.UIS_FLAG_STEPWISE), ('resident', _capi.UIS_FLAG_RESIDENT))
  return (('default', 0), ('stepwise', _capi.UIS_FLAG_STEPWISE))


@pytest.mark.parametrize('name', ['tracker_d256', 'tiny_d16'])
@pytest.mark.parametrize('beam', [10, 4, 3])
def test_a_commit_without_a_horizon_changes_no_readout(name, beam, oracle_lib):
  case = _case(name)
  reps = _replays(name, beam)
  dec = _capi.Decoder(case['params'])
  for path, flags in _paths(name):
    for chunk in (1, 7, 17):
      _transparent(dec, case['params'], case['seqs'], reps, beam, chunk, flags, (name, beam, path, chunk))
  dec.close()


def test_the_references_commits_are_the_ones_the_cases_were_chosen_for(oracle_lib):
  """tracker_d256 utterance 1 commits 40 of 60 at beams 10 and 4; tiny_d16 utterance 0 commits 12 of 23 at beam 10
  and 14 at beam 4, utterance 3 commits 12 of 19 at beam 4."""
  def committed(name, beam, u):
    ref = commit_ref.ReplaySession(_replays(name, beam)[u])
    for _ in range(len(_case(name)['seqs'][u])):
      ref.push(1)
      ref.commit()
    return ref.committed
  assert [committed('tracker_d256', b, 1) for b in (10, 4)] == [40, 40]
  assert [committed('tiny_d16', b, 0) for b in (10, 4)] == [12, 14]
  assert committed('tiny_d16', 4, 3) == 12


@pytest.mark.parametrize('name,beam,chunk', [('tracker_d64_h300', 2, 7), ('toy_d2_depth2', 3, 1)])
def test_a_commit_without_a_horizon_on_other_model_shapes(name, beam, chunk, oracle_lib):
  case = _case(name)
  dec = _capi.Decoder(case['params'])
  for flags in (0, _capi.UIS_FLAG_STEPWISE):
    _transparent(dec, case['params'], case['seqs'], _replays(name, beam), beam, chunk, flags, (name, beam, flags, chunk))
  dec.close()


def test_a_persistent_session_stays_persistent(oracle_lib):
  if not gh._whole_device():   # pylint: disable=protected-access
    pytest.skip('not a whole MI355X')
  name, beam = 'tracker_d256', 4
  case = _case(name)
  dec = _capi.Decoder(case['params'])
  for chunk in (1, 7):
    _transparent(dec, case['params'], case['seqs'], _replays(name, beam), beam, chunk, _capi.UIS_FLAG_PERSISTENT,
                 (name, beam, 'persistent', chunk))
  dec.close()
  # ... and through OnlineSession, which knows whether the library took the session as a persistent one
  model_args, _, args = uisrnn_amd.parse_arguments(['--observation_dim', '256', '--rnn_hidden_size', '512'])
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(case['params'])
  args.beam_size, args.look_ahead, args.test_iteration = beam, 1, 1
  seqs = [np.asarray(s, dtype=np.float64) for s in case['seqs']]
  offline = model.predict(seqs, args)
  with model.online(len(seqs), args, max_frames=60, persistent=True) as session:
    assert session.persistent
    for lo in range(0, 60, 7):
      session.push(_chunks(seqs, lo, 7))
      session.commit()
    assert session.persistent
    assert session.labels() == offline
    assert session.committed == [10, 40, 4]


# ---- a primed session

@functools.lru_cache(maxsize=None)
def _primed_refs(beam, chunk):
  case = _case('tiny_d16')
  model = _model('tiny_d16')
  greedy = oracle.decode(case['params'], case['seqs'], 1, 1, 1)
  plen = [6, 3, 0, 5]
  prefixes = [greedy['labels'][u][:p].astype(np.int32) for u, p in enumerate(plen)]
  out = []
  for u, p in enumerate(plen):
    seq = case['seqs'][u]
    ref = commit_ref.Session(model, beam, primed_ref.advance_forced(model, seq[:p], prefixes[u]) if p else None)
    steps = [(ref.commit(), _ref_shot(ref))]
    for lo in range(p, len(seq), chunk):
      ref.push(seq[lo:lo + chunk])
      shot = _ref_shot(ref)
      steps.append((ref.commit(), shot))
    out.append((ref, steps))
  return prefixes, out


def _ref_shot(ref):
  rows = ref.rows()
  return {'labels': ref.labels(), 'rows': [ref.final + r.tolist() for r in rows], 'scores': ref.scores(),
          'stable': ref.committed + ref.stable()}


def _against_ref(shot, u, want, beam, what):
  assert shot['labels'][u] == want['labels'], what
  assert shot['rows'][u] == want['rows'], what
  assert shot['counts'][u] == len(want['rows']), what
  assert shot['beam'][u] == _bits(primed_ref.padded_beam(want['scores'], beam)).tolist(), what
  assert shot['nb_scores'][u] == shot['beam'][u], what
  assert shot['stable'][u] == want['stable'], what


def test_prime_then_commits(oracle_lib):
  beam, chunk = 4, 1
  case = _case('tiny_d16')
  seqs = case['seqs'][:4]
  prefixes, refs = _primed_refs(beam, chunk)
  _not_vacuous([r for r, _ in refs], [len(s) for s in seqs], 'primed')
  dec = _capi.Decoder(case['params'])
  dec.stream_begin(4, beam, max(len(s) for s in seqs))
  try:
    session = _Session(dec, 4, beam)
    dec.stream_prime([s[:len(p)] if len(p) else None for s, p in zip(seqs, prefixes)], [p if len(p) else None for p in prefixes])
    pos = [len(p) for p in prefixes]
    for k in range(max(len(steps) for _, steps in refs)):   # step 0: the commit right after priming
      if k:
        dec.stream_push([s[p:p + chunk] if p < len(s) else None for s, p in zip(seqs, pos)])
        pos = [min(p + chunk, len(s)) for s, p in zip(seqs, pos)]
      shot = session.snapshot()
      out, dropped = session.commit()
      for u, (_, steps) in enumerate(refs):
        if k < len(steps):
          (want_out, want_dropped), want = steps[k]
          if pos[u]:
            _against_ref(shot, u, want, beam, ('primed', k, u))
          assert (out[u], dropped[u]) == (want_out, want_dropped), ('primed', k, u)
        else:   # the utterance has ended
          assert (out[u], dropped[u]) == ([], 0), ('primed', k, u)
    assert [len(f) for f in session.final] == [r.committed for r, _ in refs]
    assert session.snapshot()['labels'] == [r.labels() for r, _ in refs]
  finally:
    dec.stream_end()
  dec.close()


# ---- 2. horizon

@functools.lru_cache(maxsize=None)
def _horizon_refs(name, utts, beam, horizon, chunk):
  """Per utterance (session, [((labels out, dropped), readouts before the commit) per push])."""
  case = _case(name)
  out = []
  longest = max(len(case['seqs'][u]) for u in utts)
  for u in utts:
    seq = case['seqs'][u]
    ref = commit_ref.Session(_model(name), beam)
    steps = []
    for lo in range(0, longest, chunk):   # (an utterance that has ended is committed along with the others: after a
      ref.push(seq[lo:lo + chunk])        # prune the survivors may agree on more than the cut, and that is final too)
      shot = _ref_shot(ref)
      steps.append((ref.commit(horizon), shot))
    out.append((ref, steps))
  return out


def _horizon_case(dec, name, utts, beam, horizon, chunk, flags=0):
  what = (name, beam, horizon, chunk, flags)
  case = _case(name)
  seqs = [case['seqs'][u] for u in utts]
  refs = _horizon_refs(name, utts, beam, horizon, chunk)
  history = [h for r, _ in refs for h in r.history]
  assert sum(h.dropped for h in history) > 0, what                      # pruning does remove hypotheses
  if horizon > 0:   # ... and not only from the end of the beam: the survivors' gather has something to do
    assert any(h.kept != list(range(len(h.kept))) for h in history), what
  longest = max(len(s) for s in seqs)
  dec.stream_begin(len(seqs), beam, longest, flags=flags)
  try:
    session = _Session(dec, len(seqs), beam)
    for k, lo in enumerate(range(0, longest, chunk)):
      dec.stream_push(_chunks(seqs, lo, chunk))
      shot = session.snapshot()
      out, dropped = session.commit(horizon)
      for u, (_, steps) in enumerate(refs):
        (want_out, want_dropped), want = steps[k]
        _against_ref(shot, u, want, beam, what + (lo, u))
        assert (out[u], dropped[u]) == (want_out, want_dropped), what + (lo, u)
    last = session.snapshot()
    assert last['labels'] == [r.labels() for r, _ in refs], what
    assert [len(f) for f in session.final] == [r.committed for r, _ in refs], what
  finally:
    dec.stream_end()


@pytest.mark.parametrize('horizon', [8, 0])
@pytest.mark.parametrize('beam', [10, 4])
def test_a_horizon_decides_for_the_best_hypothesis(horizon, beam, oracle_lib):
  name = 'tiny_d16'
  utts = tuple(range(len(_case(name)['seqs'])))
  dec = _capi.Decoder(_case(name)['params'])
  for chunk in (1, 7):
    _horizon_case(dec, name, utts, beam, horizon, chunk)
  _horizon_case(dec, name, utts, beam, horizon, 7, flags=_capi.UIS_FLAG_STEPWISE)
  dec.close()
  if (horizon, beam) == (8, 10):   # (the CPU findings the cases rest on)
    assert sum(h.dropped for h in _horizon_refs(name, utts, 10, 8, 1)[0][0].history) == 10
  if (horizon, beam) == (0, 10):   # horizon 0 changes the final labels of utterance 3: the semantics are visible
    assert _horizon_refs(name, utts, 10, 0, 1)[3][0].labels() != nbest_ref.nbest(_replays(name, 10)[3])[0][0].tolist()


@pytest.mark.parametrize('horizon', [8, 0])
def test_a_horizon_on_the_one_launch_shape(horizon, oracle_lib):
  name, beam = 'tracker_d256', 4
  dec = _capi.Decoder(_case(name)['params'])
  for chunk in (1, 7):
    _horizon_case(dec, name, (2,), beam, horizon, chunk)
  _horizon_case(dec, name, (2,), beam, horizon, 7, flags=_capi.UIS_FLAG_RESIDENT)
  dec.close()
  if horizon == 8:
    assert sum(h.dropped for h in _horizon_refs(name, (2,), 4, 8, 1)[0][0].history) == 4


def test_after_horizon_0_a_session_is_a_session_primed_with_its_labels(oracle_lib):
  """On the device alone: collapse the beam, prime a second session with labels(), push the same frames to both."""
  name, beam, split, chunk = 'tracker_d256', 4, 11, 7
  case = _case(name)
  seqs = case['seqs']
  first, second = _capi.Decoder(case['params']), _capi.Decoder(case['params'])
  first.stream_begin(3, beam, 60)
  second.stream_begin(3, beam, 60)
  try:
    a, b = _Session(first, 3, beam), _Session(second, 3, beam)
    first.stream_push([s[:split] for s in seqs])
    _, dropped = a.commit(0)
    assert all(d > 0 for d in dropped) and first.stream_committed().tolist() == [split - 1] * 3
    shot = a.snapshot()
    assert shot['counts'] == [1, 1, 1] and shot['stable'] == [split] * 3
    second.stream_prime([s[:split] for s in seqs], [np.array(l, dtype=np.int32) for l in shot['labels']])
    assert b.snapshot() == shot
    for lo in range(split, 60, chunk):
      first.stream_push(_chunks(seqs, lo, chunk))
      second.stream_push(_chunks(seqs, lo, chunk))
      assert a.snapshot() == b.snapshot(), lo
      a.commit()
  finally:
    first.stream_end()
    second.stream_end()
  first.close()
  second.close()


# ---- 3. longer than the window

LONG_FRAMES, LONG_WINDOW, LONG_CHUNK = 400, 16, 5


@functools.lru_cache(maxsize=None)
def _long_seq():
  return np.asarray(synth.make_utterance(4242, LONG_FRAMES, 16)[0], dtype=np.float64)


def _online(beam):
  params = _case('tiny_d16')['params']
  model_args, _, args = uisrnn_amd.parse_arguments(
      ['--observation_dim', '16', '--rnn_hidden_size', str(int(params['rnn_hidden_size']))])
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params)
  args.beam_size, args.look_ahead, args.test_iteration = beam, 1, 1
  return model, args


def _table_lengths(err):
  return [int(line.split('prior_table_entries ')[1].split()[0]) for line in err.splitlines() if 'prior_table_entries' in line]


def test_a_greedy_stream_longer_than_the_window_is_the_offline_decode(oracle_lib, monkeypatch, capfd):
  monkeypatch.setenv('UIS_COMMIT_TRACE', '1')
  seq = _long_seq()
  model, args = _online(1)
  offline = model.predict(seq, args)
  commits = 0
  with model.online(1, args, LONG_WINDOW) as session:
    for lo in range(0, LONG_FRAMES, LONG_CHUNK):
      session.push([seq[lo:lo + LONG_CHUNK]])
      commits += 1 if session.commit()[0] else 0
      assert session._decoder.stream_received()[0] <= 1   # pylint: disable=protected-access
    assert session.labels() == [offline]
    assert session.committed == [LONG_FRAMES] and commits == LONG_FRAMES // LONG_CHUNK
    assert session.stable_frames() == [LONG_FRAMES]
  lengths = _table_lengths(capfd.readouterr().err)
  # 18 entries at uis_stream_begin, doubled whenever (frames received) + window + 2 passes the length
  assert sorted(set(lengths)) == [36, 72, 144, 288, 576] and lengths == sorted(lengths), sorted(set(lengths))


@pytest.mark.parametrize('beam', [4, 10])
def test_a_session_with_a_horizon_runs_on_for_ever(beam, oracle_lib, monkeypatch, capfd):
  monkeypatch.setenv('UIS_COMMIT_TRACE', '1')
  seq = _long_seq()
  ref, shots = commit_ref.run(_model('tiny_d16'), seq, beam, LONG_CHUNK, horizon=8, auto_window=LONG_WINDOW)
  assert max(h.have for h in ref.history) <= LONG_WINDOW and len(ref.history) >= 40
  model, args = _online(beam)
  with model.online(1, args, LONG_WINDOW, horizon=8) as session:
    for k, lo in enumerate(range(0, LONG_FRAMES, LONG_CHUNK)):
      session.push([seq[lo:lo + LONG_CHUNK]])
      assert session.committed == [shots[k]['committed']], lo
      if k % 8 == 7 or lo + LONG_CHUNK >= LONG_FRAMES:
        assert session.labels() == [shots[k]['labels']], lo
        rows, scores = session.nbest()[0]
        assert rows == [ref.final[:shots[k]['committed']] + r.tolist() for r in shots[k]['rows']], lo
        assert _bits(scores).tolist() == _bits(shots[k]['scores']).tolist(), lo
        assert session.stable_frames() == [shots[k]['stable']], lo
    assert session.commit(8) == [ref.commit(8)[0]]   # the stream ends: what the horizon still decides
    assert session.committed == [ref.committed] == [{4: 398, 10: 394}[beam]]
    assert session.labels() == [ref.labels()]
    with pytest.raises(ValueError, match=r'horizon \+ chunk \+ 1 = 25'):
      session.push([np.zeros((16, 16))])
  lengths = _table_lengths(capfd.readouterr().err)
  assert sorted(set(lengths)) == [36, 72, 144, 288, 576] and lengths == sorted(lengths), sorted(set(lengths))


def test_without_a_horizon_the_window_fills_up_and_a_commit_with_one_frees_it(oracle_lib):
  beam = 4
  seq = _long_seq()
  ref = commit_ref.Session(_model('tiny_d16'), beam)
  model, args = _online(beam)
  refused_at = None
  with model.online(1, args, LONG_WINDOW) as session:
    for lo in range(0, LONG_FRAMES, LONG_CHUNK):
      part = seq[lo:lo + LONG_CHUNK]
      if refused_at is None and ref.have + len(part) > LONG_WINDOW:   # the stable prefix has stopped moving
        refused_at = lo
        before = (session.labels(), session.nbest(), session.stable_frames(), session.committed)
        with pytest.raises(_capi.HipLibraryError, match='uis_stream_commit') as err:
          session.push([part])
        assert err.value.status == _capi.UIS_ERR_INVALID_ARG
        assert (session.labels(), session.nbest(), session.stable_frames(), session.committed) == before
        assert session.commit(8) == [ref.commit(8)[0]]
      session.push([part])
      ref.push(part)
      assert session.commit(None if refused_at is None else 8) == [ref.commit(None if refused_at is None else 8)[0]], lo
    assert refused_at is not None and 0 < refused_at < LONG_FRAMES - 2 * LONG_WINDOW
    assert session.labels() == [ref.labels()]
    assert session.committed == [ref.committed]
    assert _bits(session.nbest()[0][1]).tolist() == _bits(ref.scores()).tolist()


# ---- 4. the edges of the two kernels

@functools.lru_cache(maxsize=None)
def _edge_stable(beam):
  """The stable prefix of the long stream after 1 .. LONG_FRAMES frames."""
  rep = nbest_ref.replay(_case('tiny_d16')['params'], _long_seq(), beam)
  return [nbest_ref.common_prefix(nbest_ref.nbest(rep, upto=n)[0]) for n in range(1, LONG_FRAMES + 1)]


def _edge_plan(beam, retained):
  """The shortest prefix of the long stream, N frames, whose stable prefix is at most N - retained with N - retained
  even and positive: commit(horizon=retained) then commits exactly N - retained and moves `retained` rows."""
  stable = _edge_stable(beam)
  for n in range(retained + 2, LONG_FRAMES - 8, 2):
    if stable[n - 1] <= n - retained:
      return n
  raise AssertionError('no such prefix')


# (beam, rows retained): words moved = beam * rows
MOVE_EDGES = [
    (3, 0), (3, 1), (10, 1), (10, 0),
    (11, (MOVE_TILE_WORDS - 1) // 11),          # 1023 words: one below the tile
    (4, MOVE_TILE_WORDS // 4),                  # 1024 words: the tile
    (5, (MOVE_TILE_WORDS + 1) // 5),            # 1025 words: one above
    (3, 102), (3, 103),                         # rows of 12 bytes
    (10, MOVE_TILE_WORDS // 10), (10, MOVE_TILE_WORDS // 10 + 1),   # 1020 and 1030 words
    (10, 2 * MOVE_TILE_WORDS // 10 + 1),        # 2050 words: two tiles and a tail of two words
]


def test_the_edge_cases_reach_both_access_widths(oracle_lib):
  """k_commit_move uses 16-byte accesses where source and destination allow it (committed * beam a multiple of 4
  words) and 4-byte ones otherwise: both happen, at one tile and at more."""
  assert (11 * ((MOVE_TILE_WORDS - 1) // 11), 4 * (MOVE_TILE_WORDS // 4), 5 * ((MOVE_TILE_WORDS + 1) // 5)) == (1023, 1024, 1025)
  wide, narrow = set(), set()
  for beam, retained in MOVE_EDGES:
    committed = _edge_plan(beam, retained) - retained
    (wide if committed * beam % 4 == 0 else narrow).add(-(-beam * retained // MOVE_TILE_WORDS))
  assert {1, 2} <= wide and {1, 2} <= narrow, (wide, narrow)


@pytest.mark.parametrize('beam,retained', MOVE_EDGES)
def test_the_move_at_its_tile_edges(beam, retained, oracle_lib):
  n = _edge_plan(beam, retained)
  seq = _long_seq()
  ref = commit_ref.Session(_model('tiny_d16'), beam)
  ref.push(seq[:n])
  dec = _capi.Decoder(_case('tiny_d16')['params'])
  dec.stream_begin(2, beam, n + 8)
  try:
    session = _Session(dec, 2, beam)
    dec.stream_push([seq[:n], seq[:3]])          # (a neighbour that commits 2 of 3: retained 1)
    before = session.snapshot()
    _against_ref(before, 0, _ref_shot(ref), beam, 'before')
    out, dropped = session.commit([retained, 1])
    want_out, want_dropped = ref.commit(retained)
    assert ref.history[-1].committed == n - retained >= 2 and ref.have == retained
    assert (out[0], dropped[0]) == (want_out, want_dropped)
    assert len(out[1]) == 2 and dec.stream_received().tolist() == [retained, 1]
    after = session.snapshot()
    assert after['labels'] == before['labels']
    if retained:
      _against_ref(after, 0, _ref_shot(ref), beam, 'after')
    dec.stream_push([seq[n:n + 8], None])        # the records that moved are walked again, with new ones on top
    ref.push(seq[n:n + 8])
    _against_ref(session.snapshot(), 0, _ref_shot(ref), beam, 'later')
  finally:
    dec.stream_end()
  dec.close()


@pytest.mark.parametrize('beam', [1, 3, 10])
def test_small_commits(beam, oracle_lib):
  """Committed 2 with retained 0 and 1, an odd stable prefix (it commits stable - 1), beam sizes 1, 3 and 10."""
  case = _case('tiny_d16')
  seqs = case['seqs'][:4]
  reps = _replays('tiny_d16', beam) if beam > 1 else [nbest_ref.replay(case['params'], s, 1) for s in case['seqs']]
  dec = _capi.Decoder(case['params'])
  dec.stream_begin(4, beam, 32)
  try:
    session = _Session(dec, 4, beam)
    refs = [commit_ref.ReplaySession(r) for r in reps[:4]]
    odd = 0
    for counts in ([2, 3, 1, 0], [1, 0, 2, 5], [3, 3, 3, 3], [0, 1, 0, 2]):
      pos = [r.received for r in refs]
      dec.stream_push([s[p:p + n] if n else None for s, p, n in zip(seqs, pos, counts)])
      for r, n in zip(refs, counts):
        r.push(n)
      before = session.snapshot()
      out, dropped = session.commit()
      want = [r.commit()[0] for r in refs]
      assert out == want and dropped == [0] * 4, counts
      odd += sum(1 for r in refs if r.history and r.history[-1].stable % 2 == 1 and r.history[-1].committed == r.history[-1].stable - 1)
      lab = dec.stream_labels()[0]
      assert [session.final[u] + lab[u].tolist() for u in range(4)] == before['labels']
    if beam == 1:   # greedy: everything received is stable
      assert [h.committed for h in refs[0].history][:2] == [2, 0] and refs[0].history[0].have == 2    # committed 2, retained 0
      assert refs[1].history[0].have == 3 and refs[1].history[0].committed == 2                      # committed 2, retained 1
      assert session.final == [r.final for r in refs] and [len(f) for f in session.final] == [6, 6, 6, 10]
    assert odd >= 1
  finally:
    dec.stream_end()
  dec.close()


def test_excluded_utterances_commit_nothing_while_their_neighbours_commit(oracle_lib):
  """No frames, an emptied beam (tests/hostile.py's overflow regime: a frame whose every candidate is +inf) and the
  cluster cap: left alone, whatever the horizon."""
  beam, cap = 3, 2
  case = hostile.build('overflow', 16, 8, 1, lengths=(12, 9, 15, 8, 14, 11))
  seqs = list(case.seqs) + [np.zeros((0, 16))]
  ref = oracle.decode(case.params, case.seqs, beam, 1, 1)
  assert ref['max_clusters'].tolist() == [2, 2, 2, 2, 2, 3]                 # utterance 5 needs a third cluster
  assert [bool((l == -1).all()) for l in ref['labels']] == [False, False, True, True, False, False]   # 2 and 3 lose their beam
  excluded, others = (2, 3, 5, 6), (0, 1, 4)
  reps = {u: nbest_ref.replay(case.params, case.seqs[u], beam) for u in others}
  dec = _capi.Decoder(case.params)
  dec.stream_begin(7, beam, 16, max_clusters=cap)
  try:
    session = _Session(dec, 7, beam)
    dec.stream_push([s if len(s) else None for s in seqs])
    before = session.snapshot()
    assert before['overflow'] == [0, 0, 0, 0, 0, 1, 0] and before['counts'] == [3, 3, 0, 0, 3, 0, 0]
    out, dropped = session.commit()
    refs = {u: commit_ref.ReplaySession(reps[u]) for u in others}
    for u in others:
      refs[u].push(len(seqs[u]))
      assert out[u] == refs[u].commit()[0] and len(out[u]) >= 6, u
    for u in excluded:
      assert out[u] == [] and dropped[u] == 0, u
    after = session.snapshot()
    assert after == before
    out, dropped = session.commit(0)
    assert all(out[u] == [] and dropped[u] == 0 for u in excluded)
    assert all(dropped[u] == 2 for u in others) and dec.stream_received().tolist()[:2] == [0, 1]
    last = session.snapshot()
    assert last['labels'] == before['labels'] and last['overflow'] == before['overflow']
    assert [last['counts'][u] for u in excluded] == [0, 0, 0, 0]
    assert [last['beam'][u] for u in excluded] == [before['beam'][u] for u in excluded]
  finally:
    dec.stream_end()
  dec.close()


# ---- 5. refusals, stale memory

def test_refusals_leave_the_session_as_it_was(oracle_lib):
  name, beam = 'tiny_d16', 4
  case = _case(name)
  seqs = case['seqs'][:4]
  reps = _replays(name, beam)[:4]
  dec = _capi.Decoder(case['params'])
  counts = np.zeros(4, dtype=np.int32)
  labels = np.full(64, -7, dtype=np.int32)
  committed = np.zeros(4, dtype=np.int64)

  def raw_commit(capacity):
    return dec._lib.uis_stream_commit(dec._handle, None, labels.ctypes.data_as(_i32p), capacity,   # pylint: disable=protected-access
                                      counts.ctypes.data_as(_i32p), None)

  # no session open
  assert raw_commit(64) == _capi.UIS_ERR_INVALID_ARG
  assert dec._lib.uis_stream_committed(dec._handle, committed.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == _capi.UIS_ERR_INVALID_ARG  # pylint: disable=protected-access
  dec.stream_begin(4, beam, 32)
  try:
    session = _Session(dec, 4, beam)
    dec.stream_push([s[:12] for s in seqs])
    before = session.snapshot()
    have = int(dec.stream_received().sum())
    # capacity too small
    assert raw_commit(have - 1) == _capi.UIS_ERR_INVALID_ARG
    assert (labels == -7).all() and dec.stream_committed().tolist() == [0] * 4
    assert session.snapshot() == before
    refs = [commit_ref.ReplaySession(r) for r in reps]
    for r, s in zip(refs, seqs):
      r.push(min(12, len(s)))
    out, _ = session.commit()
    assert out == [r.commit()[0] for r in refs] and sum(len(o) for o in out) >= 8
    assert session.snapshot() == before
  finally:
    dec.stream_end()
  # prime after a full commit: the window is empty, the utterance has received frames all the same
  frames, offsets = oracle.pack([seqs[0]])
  off = dec.decode(frames, offsets, 1, 1, 1, want_beam_scores=True)
  dec.stream_begin(1, 1, 32)
  try:
    session = _Session(dec, 1, 1)
    dec.stream_push([seqs[0][:4]])
    assert session.commit()[0] == [off['labels'][:4].tolist()] and dec.stream_received().tolist() == [0]
    with pytest.raises(_capi.HipLibraryError, match='already received') as err:
      dec.stream_prime([seqs[0][:2]], [np.zeros(2, dtype=np.int32)])
    assert err.value.status == _capi.UIS_ERR_INVALID_ARG
    dec.stream_push([seqs[0][4:]])
    shot = session.snapshot()
    assert shot['labels'] == [off['labels'].tolist()] and shot['scores'] == _bits(off['scores']).tolist()
    assert shot['beam'] == _bits(off['beam_scores']).tolist()
  finally:
    dec.stream_end()
  dec.close()


@pytest.mark.parametrize('word', WORDS)
def test_no_output_depends_on_stale_memory(word, oracle_lib, monkeypatch):
  monkeypatch.setenv(KNOB, word)
  monkeypatch.delenv('UIS_NO_ARENA', raising=False)
  name = 'tiny_d16'
  case = _case(name)
  dec = _capi.Decoder(case['params'])
  for flags in (0, _capi.UIS_FLAG_STEPWISE):
    _transparent(dec, case['params'], case['seqs'], _replays(name, 4), 4, 7, flags, (word, flags))
  _horizon_case(dec, name, tuple(range(len(case['seqs']))), 10, 8, 1)
  dec.close()
  name = 'tracker_d256'
  case = _case(name)
  dec = _capi.Decoder(case['params'])
  _transparent(dec, case['params'], case['seqs'], _replays(name, 4), 4, 7, 0, (word, name))
  _horizon_case(dec, name, (2,), 4, 8, 7)
  dec.close()
