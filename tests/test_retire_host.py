"""Speaker retirement's CPU side: the restatement the GPU tests compare with, the id map, the Python layer's checks.

tests/retire_ref.py restates a session that retires clusters: commit_ref's Session plus retirable() / retire(R) as
list surgery on primed_ref.Hypothesis.  Held here to what makes it a reference -- retiring nothing changes nothing,
a retired cluster changes no remaining cluster's likelihood and the priors are the formula with the reduced block
sum, and nothing in use is ever retirable -- and the map between the library's present indices and the ids a
session hands out is walked through sequences of retirements.  No GPU needed.
"""

import math
import os
import subprocess

import numpy as np
import pytest

import golden_util
import primed_ref
import retire_ref
import uisrnn_amd
from oracle import oracle
from uisrnn_amd import _capi
from uisrnn_amd import build as lib_build
from uisrnn_amd import uisrnn as host


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


speaker_walk = retire_ref.speaker_walk


def _state(hyp):
  return ([m.tobytes() for m in hyp.means], [np.asarray(h).tobytes() for h in hyp.hids], hyp.counts, hyp.blk, hyp.last,
          hyp.sumblk, int(_bits(hyp.score)[0]), hyp.trace)


def _runs(name, scale):
  """A session over a walk through 30 speakers that commits with horizon 8 every 8 frames; yields it after each."""
  params = golden_util.load_case(name)['params']
  seq = speaker_walk(1, params['observation_dim'], 30, 3, 90, scale=scale)
  session = retire_ref.Session(params, 4)
  for t in range(len(seq)):
    session.push(seq[t:t + 1])
    if t % 8 == 7:
      session.commit(8)
      yield session, seq[min(t + 1, len(seq) - 1)]


CASES = [('tiny_d16', 3.0), ('toy_d2_depth2', 1.0)]


@pytest.mark.parametrize('name,scale', CASES)
def test_retiring_nothing_is_the_identity(name, scale, oracle_lib):
  for session, _ in _runs(name, scale):
    before = [_state(h) for h in session.beam]
    assert session.retire([]) == []
    assert [_state(h) for h in session.beam] == before and session.gone == []


@pytest.mark.parametrize('name,scale', CASES)
def test_a_retired_cluster_changes_no_likelihood_and_the_priors_follow_the_reduced_sum(name, scale, oracle_lib):
  found = 0
  for session, x in _runs(name, scale):
    able = session.retirable()
    if not able:
      continue
    found += 1
    model = session.model
    x = np.asarray(x, dtype=np.float32)
    old = [h.copy() for h in session.beam]
    R = able[::2] if len(able) > 1 else able
    session.retire(R)
    for h0, h1 in zip(old, session.beam):
      gone_blocks = sum(h0.blk[k] for k in R)
      assert h1.sumblk == h0.sumblk - gone_blocks and len(h1.means) == len(h0.means) - len(R)
      assert _bits(h1.score) == _bits(h0.score)
      kept = [k for k in range(len(h0.means)) if k not in R]
      for j, k in enumerate(kept):
        assert h1.means[j] is h0.means[k] and h1.hids[j] is h0.hids[k]   # the same state: the same weighted MSE
        assert (h1.counts[j], h1.blk[j]) == (h0.counts[k], h0.blk[k])
        mse = oracle.weighted_mse(model.params, h0.means[k], x)
        if k == h0.last:
          assert h1.last == j
          prior = model.lp_stay
        else:
          prior = model.lp_sw + math.log(float(h0.blk[k])) - math.log(float(h0.sumblk - gone_blocks) + model.alpha)
        want = np.float32(h0.score + np.float32(np.float64(mse) - prior))
        assert _bits(h1.candidate(model, x, j)) == _bits(want), (k, j)
      prior = model.lp_sw + model.l_alpha - math.log(float(h0.sumblk - gone_blocks) + model.alpha)
      mse = oracle.weighted_mse(model.params, model.m0, x)
      assert _bits(h1.candidate(model, x, len(kept))) == _bits(np.float32(h0.score + np.float32(np.float64(mse) - prior)))
  assert found > 0   # (not vacuous: the walk does leave clusters behind)


@pytest.mark.parametrize('name,scale', CASES)
def test_nothing_in_use_is_retirable(name, scale, oracle_lib):
  found = 0
  for session, _ in _runs(name, scale):
    able = set(session.retirable())
    found += len(able)
    for h, row in zip(session.beam, session.rows()):
      assert not able & set(row.tolist()) and h.last not in able and all(k < len(h.means) for k in able)
  assert found > 0


def test_a_session_that_never_committed_has_nothing_retirable(oracle_lib):
  params = golden_util.load_case('toy_d2_depth2')['params']
  session = retire_ref.Session(params, 4)
  assert session.retirable() == [] and session.K() == 0
  session.push(speaker_walk(1, 2, 30, 3, 40))
  assert session.K() > 1 and session.retirable() == []


def test_the_id_map():
  assert [retire_ref.to_global(j, []) for j in range(4)] == [0, 1, 2, 3]
  assert [retire_ref.to_global(j, [1, 3]) for j in range(4)] == [0, 2, 4, 5]
  assert retire_ref.to_global(-1, [0]) == -1
  assert host._stable_ids([1, 3], 4) == [0, 2, 4, 5] and host._stable_ids([], 3) == [0, 1, 2]
  # two retirements in a row, then a new speaker: ids 0 .. 5 exist, present indices 0 .. 5
  gone = []
  ids = [retire_ref.to_global(k, gone) for k in (1, 3)]           # the first retirement: present 1 and 3
  gone = sorted(gone + ids)
  assert ids == [1, 3] and [retire_ref.to_global(j, gone) for j in range(4)] == [0, 2, 4, 5]
  ids = [retire_ref.to_global(k, gone) for k in (0, 2)]           # the second: present 0 and 2 are ids 0 and 4
  gone = sorted(gone + ids)
  assert ids == [0, 4] and gone == [0, 1, 3, 4]
  assert [retire_ref.to_global(j, gone) for j in range(3)] == [2, 5, 6]   # the next new cluster is index 2: id 6, unused
  assert [retire_ref.to_local(g, gone) for g in (2, 5, 6)] == [0, 1, 2]
  for seed in range(20):
    rng = np.random.default_rng(seed)
    gone, alive, nxt = [], list(range(5)), 5
    for _ in range(12):
      if alive and rng.random() < 0.6:
        pick = sorted(rng.choice(len(alive), size=int(rng.integers(1, len(alive) + 1)), replace=False).tolist())
        ids = [retire_ref.to_global(k, gone) for k in pick]
        assert ids == [alive[k] for k in pick]
        gone = sorted(gone + ids)
        alive = [a for a in alive if a not in ids]
      else:
        alive.append(nxt)     # a new speaker takes the next index: an id nobody ever had
        nxt += 1
      assert [retire_ref.to_global(j, gone) for j in range(len(alive))] == alive == host._stable_ids(gone, len(alive))
      assert [retire_ref.to_local(g, gone) for g in alive] == list(range(len(alive)))


class _NoDevice:
  """A decoder that fails the test when anything reaches it."""

  def __getattr__(self, name):
    raise AssertionError('the decoder was reached: ' + name)


class _StandIn:
  """A decoder without a device: K grows by one per frame, everything below `active` is retirable."""

  def __init__(self, n_utt, cap):
    self.k, self.cap, self.active = [0] * n_utt, cap, 2
    self.have = np.zeros(n_utt, dtype=np.int64)
    self.calls = []

  def stream_received(self):
    return self.have.copy()

  def stream_push(self, chunks):
    for u, c in enumerate(chunks):
      self.k[u] += 0 if c is None else len(c)
      assert self.k[u] <= self.cap
    self.calls.append('push')

  def stream_commit(self, horizon):
    self.calls.append(('commit', horizon))
    return [np.zeros(0, dtype=np.int32) for _ in self.k], np.zeros(len(self.k), dtype=np.int32)

  def stream_retire(self, which=None, clusters=None):
    self.calls.append(('retire', which, clusters))
    retired = [np.asarray(c if c is not None else [], dtype=np.int32) for c in clusters]
    able = [np.arange(max(k - self.active, 0), dtype=np.int32) for k in self.k]
    for u, r in enumerate(retired):
      assert set(r.tolist()) <= set(able[u].tolist())
      self.k[u] -= len(r)
    return {'retired': retired, 'K': np.array(self.k, dtype=np.int32), 'retirable': able, 'max_clusters': self.cap}


def _session(n_utt, decoder, retire_at=None, retire_to=None, cap=16):
  model_args, _, _ = uisrnn_amd.parse_arguments([])
  model_args.observation_dim = 4
  session = host.OnlineSession.__new__(host.OnlineSession)  # (no handle)
  session._model = uisrnn_amd.UISRNN(model_args)
  session._num_utterances = n_utt
  session._beam_size = 2
  session._decoder = decoder
  session._horizon, session._max_frames = None, 1000
  session._final = [[] for _ in range(n_utt)]
  session._bound = [0] * n_utt
  session._seen = [{} for _ in range(n_utt)]
  session._set_retire_policy(retire_at, retire_to, cap)
  return session


def test_the_python_argument_checks_raise_before_any_device_call():
  session = _session(2, _NoDevice())
  with pytest.raises(ValueError, match='not in'):
    session.retire([2])
  with pytest.raises(ValueError, match='given twice'):
    session.retire([1, 1])
  with pytest.raises(ValueError, match='exclude each other'):
    session.retire([0], clusters=[[0], None])
  with pytest.raises(ValueError, match='per utterance'):
    session.retire(clusters=[[0]])
  with pytest.raises(ValueError, match='non-negative integer'):
    session.retire(clusters=[[-1], None])
  with pytest.raises(ValueError, match='given twice'):
    session.retire(clusters=[[1, 1], None])
  session._gone = [[1], []]
  with pytest.raises(ValueError, match='already retired'):
    session.retire(clusters=[[1], None])
  for bad in (dict(retire_at=0), dict(retire_at=17), dict(retire_at=True), dict(retire_at=8, retire_to=8),
              dict(retire_at=8, retire_to=-1), dict(retire_to=2), dict(retire_at=2.5)):
    with pytest.raises(ValueError, match='retire_at|retire_to'):
      _session(1, _NoDevice(), **bad)
  with pytest.raises(ValueError, match='retire_at must be an integer'):
    host.OnlineSession(None, 1, None, 16, retire_at=-1)
  session = _session(1, _NoDevice(), retire_at=12)
  assert (session._retire_at, session._retire_to) == (12, 6)
  with pytest.raises(ValueError, match='too long for retire_at'):
    session.push([np.zeros((5, 4))])   # max_clusters - retire_at = 4


def test_the_automatic_policy_waits_for_its_bound_and_keeps_under_the_cap():
  dec = _StandIn(2, 16)
  session = _session(2, dec, retire_at=12, retire_to=5)
  for _ in range(3):
    session.push([np.zeros((4, 4)), np.zeros((1, 4))])
  assert dec.calls == ['push'] * 3 and session._bound == [12, 3]   # below retire_at: no device call but the pushes
  session.push([np.zeros((4, 4)), np.zeros((1, 4))])
  assert dec.calls[3][0] == 'commit' and dec.calls[4][0] == 'retire' and dec.calls[4][2] == [None, None]   # the query
  assert dec.calls[5][0] == 'retire' and dec.calls[5][2][1] is None and dec.calls[5][2][0] == list(range(7))
  assert dec.k == [9, 4] and session._bound == [9, 4] and session._gone == [list(range(7)), []]
  assert session._ids(0, np.arange(3)) == [7, 8, 9] and session._ids(1, np.arange(3)) == [0, 1, 2]
  dec.active = 16   # everybody talks inside the window: nothing retirable
  session.push([np.zeros((3, 4)), None])
  session.push([np.zeros((4, 4)), None])     # 12 live speakers and four frames: 16 clusters at the most, they fit
  assert dec.k[0] == 16 and session._bound[0] == 16
  with pytest.raises(RuntimeError, match='utterance 0'):
    session.push([np.zeros((1, 4)), None])   # one frame more could pass max_clusters
  assert dec.k[0] == 16 and dec.calls[-1][0] == 'retire'   # (the query; the push never reached the decoder)


def test_restart_clears_the_id_map():
  class _Restart(_StandIn):
    def stream_restart(self, which):
      n = len(which)
      return ([np.array([1, 0], dtype=np.int32) if w else np.zeros(0, dtype=np.int32) for w in which],
              np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int32), 0)
  session = _session(2, _Restart(2, 16))
  session._gone = [[0, 2], [1]]
  session._final = [[0, 1, 2], [5]]
  out = session.restart([0])
  assert out[0][0] == [0, 1, 2, 3, 1] and out[1] is None   # present 1, 0 -> ids 3, 1
  assert session._gone == [[], [1]] and session._final == [[], [5]]


def test_the_symbols_are_declared_bound_and_exported():
  root = os.path.join(os.path.dirname(golden_util.GOLDEN_DIR), '..')
  header = open(os.path.join(root, 'include', 'uisrnn_hip.h')).read()
  assert 'int32_t uis_stream_retire(uis_handle* h, const int32_t* which, const int64_t* offsets, const int32_t* clusters,' in header
  assert '#define UIS_ABI_VERSION 6' in header
  assert 'uis_stream_retire' in _capi.EXPORTED_SYMBOLS
  assert hasattr(_capi.Decoder, 'stream_retire') and hasattr(host.OnlineSession, 'retire') and hasattr(host.StreamPool, 'retire')
  lib = lib_build.OUTPUT
  if not os.path.exists(lib):
    lib = lib_build.build()
  symbols = subprocess.run(['nm', '-D', '--defined-only', lib], check=True, capture_output=True, text=True).stdout
  assert 'uis_stream_retire' in {line.split()[-1] for line in symbols.splitlines() if line.strip()}
