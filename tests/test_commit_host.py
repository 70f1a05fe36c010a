"""Session commits' CPU side: the restatement the GPU tests compare with, and the Python layer's bookkeeping.

tests/commit_ref.py restates a session that commits: primed_ref's beam search from a beam, plus the cut / prune /
commit rule.  Checked here against nbest_ref's replay of the oracle's candidate scores (without a horizon a commit
changes no readout), against a chain of primed_ref.primed_decode calls (horizon 0 after every push IS priming with
the best labels so far), and for the invariant that makes it useful: committed labels followed by the window's are
the best trace.  No GPU needed.
"""

import functools
import os
import subprocess

import numpy as np
import pytest

import commit_ref
import golden_util
import nbest_ref
import primed_ref
import uisrnn_amd
from uisrnn_amd import _capi
from uisrnn_amd import build as lib_build
from uisrnn_amd import uisrnn as host


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(name):
  return golden_util.load_case(name)


@pytest.mark.parametrize('beam', [10, 4, 3])
@pytest.mark.parametrize('chunk', [1, 7])
def test_without_a_horizon_every_readout_is_the_replay(beam, chunk, oracle_lib):
  case = _case('tiny_d16')
  moved = 0
  for u, seq in enumerate(case['seqs']):
    rep = nbest_ref.replay(case['params'], seq, beam)
    session, shots = commit_ref.run(case['params'], seq, beam, chunk)
    upto = 0
    for shot in shots:
      upto = min(upto + chunk, seq.shape[0])
      rows, scores = nbest_ref.nbest(rep, upto=upto)
      done = shot['committed']
      assert np.array_equal(shot['rows'], rows[:, done:]), (u, upto)
      assert np.array_equal(_bits(shot['scores']), _bits(scores)), (u, upto)
      assert shot['labels'] == rows[0].tolist(), (u, upto)
      assert shot['stable'] == nbest_ref.common_prefix(rows), (u, upto)
      assert all(rows[k][:done].tolist() == session.final[:done] for k in range(rows.shape[0])), (u, upto)
    assert all(h.dropped == 0 and h.committed == h.stable & ~1 for h in session.history), u
    moved += session.committed
  assert moved > 0   # (not vacuous: tiny_d16's stable prefix does advance)


@pytest.mark.parametrize('beam', [10, 4])
def test_horizon_0_after_every_push_is_a_chain_of_primed_decodes(beam, oracle_lib):
  case = _case('tiny_d16')
  chunk = 3
  for u, seq in enumerate(case['seqs'][:3]):
    session = commit_ref.Session(case['params'], beam)
    labels = []
    for t0 in range(0, seq.shape[0], chunk):
      t1 = min(t0 + chunk, seq.shape[0])
      session.push(seq[t0:t1])
      want = primed_ref.primed_decode(case['params'], seq[:t1], labels, beam)
      assert np.array_equal(np.array([h.trace for h in session.beam]), want['labels']), (u, t1)
      assert np.array_equal(_bits(session.scores()), _bits(want['scores'])), (u, t1)
      out, dropped = session.commit(0)
      assert len(session.beam) == 1 and dropped == want['labels'].shape[0] - 1, (u, t1)
      assert len(out) == session.history[-1].committed == (session.history[-1].have & ~1), (u, t1)
      labels = session.labels()
      assert labels == want['labels'][0].tolist(), (u, t1)


@pytest.mark.parametrize('horizon', [None, 8, 0])
def test_committed_labels_then_the_window_are_the_best_trace(horizon, oracle_lib):
  case = _case('tiny_d16')
  pruned = 0
  for u, seq in enumerate(case['seqs']):
    session, _ = commit_ref.run(case['params'], seq, 10, 1, horizon=horizon)
    assert session.final + session.rows()[0].tolist() == list(session.beam[0].trace), u
    assert session.committed % 2 == 0 and len(session.final) == session.committed, u
    for h in session.history:
      assert h.kept[0] == 0 and h.dropped == (0 if h.cut == h.stable else h.dropped), u
      if horizon is not None:
        assert h.have - h.committed <= horizon + 1, (u, h)   # the bound on the delay: the even rounding costs one frame
    pruned += sum(h.dropped for h in session.history)
  assert (pruned > 0) == (horizon is not None)


def test_the_window_of_an_automatic_session_is_horizon_plus_chunk_plus_1(oracle_lib):
  case = _case('tiny_d16')
  for chunk, window in ((1, 10), (7, 16)):
    session, _ = commit_ref.run(case['params'], case['seqs'][0], 4, chunk, horizon=8, auto_window=window)
    assert session.history, chunk
    assert max(h.have for h in session.history) <= window


class _StandIn:
  """A decoder that records what reaches it (no library, no device): a window of `have` frames whose labels are
  their own positions in the stream and whose stable prefix is 0; commit applies the cut rule to that."""

  def __init__(self, n_utt):
    self.have = np.zeros(n_utt, dtype=np.int64)
    self.done = np.zeros(n_utt, dtype=np.int64)
    self.horizons = []

  def stream_received(self):
    return self.have.copy()

  def stream_committed(self):
    return self.done.copy()

  def stream_push(self, chunks):
    for u, c in enumerate(chunks):
      self.have[u] += 0 if c is None else len(c)

  def stream_commit(self, horizon):
    self.horizons.append(horizon)
    out = []
    for u in range(len(self.have)):
      cut = 0 if horizon is None or horizon[u] < 0 else max(int(self.have[u]) - horizon[u], 0)
      c = cut & ~1
      out.append(np.arange(self.done[u], self.done[u] + c, dtype=np.int32))
      self.done[u] += c
      self.have[u] -= c
    return out, np.zeros(len(self.have), dtype=np.int32)

  def stream_labels(self):
    per_utt = [np.arange(self.done[u], self.done[u] + self.have[u], dtype=np.int32) for u in range(len(self.have))]
    return per_utt, None, np.zeros(len(self.have), dtype=np.int32), 0

  def stream_nbest(self, n_best):
    labels = [np.tile(row, (n_best, 1)) for row in self.stream_labels()[0]]
    return {'labels': labels, 'scores': np.zeros((len(labels), n_best), dtype=np.float32),
            'counts': np.full(len(labels), n_best, dtype=np.int32), 'stable': np.minimum(self.have, 1), 'status': 0}


def _session(n_utt, max_frames, horizon=None, dim=4):
  model_args, _, _ = uisrnn_amd.parse_arguments([])
  model_args.observation_dim = dim
  session = host.OnlineSession.__new__(host.OnlineSession)  # (no handle)
  session._model = uisrnn_amd.UISRNN(model_args)
  session._num_utterances = n_utt
  session._beam_size = 2
  session._decoder = _StandIn(n_utt)
  session._horizon, session._max_frames = horizon, max_frames
  session._final = [[] for _ in range(n_utt)]
  return session


def test_online_session_keeps_the_committed_labels():
  session = _session(2, 100)
  session.push([np.zeros((9, 4)), np.zeros((4, 4))])
  before = session.labels()
  assert session.commit([3, None]) == [[0, 1, 2, 3, 4, 5], []]
  assert session._decoder.horizons == [[3, -1]]
  assert session.committed == [6, 0]
  assert session.labels() == before == [list(range(9)), list(range(4))]
  assert session.nbest(2)[0][0] == [list(range(9))] * 2
  assert session.stable_frames() == [7, 1]
  assert session.commit() == [[], []] and session._decoder.horizons[-1] is None
  assert session.commit(0) == [[6, 7], [0, 1, 2, 3]] and session._decoder.horizons[-1] == [0, 0]
  assert session.labels() == before
  with pytest.raises(ValueError, match='non-negative'):
    session.commit(-1)
  with pytest.raises(ValueError, match='one horizon'):
    session.commit([1])
  with pytest.raises(ValueError, match='already received 8 frames'):   # the 8 committed ones: also with an emptied window
    session._decoder.have[0] = 0
    session.prime([np.zeros((2, 4)), None], [[0, 0], None])


def test_a_session_with_a_horizon_commits_when_a_push_does_not_fit():
  session = _session(1, 16, horizon=8)
  for _ in range(2):
    session.push([np.zeros((7, 4))])
  assert not session._decoder.horizons            # 14 of 16: nothing automatic yet
  session.push([np.zeros((7, 4))])                # 21 > 16: commit(8) takes 6 of the 14, then 7 more
  assert session._decoder.horizons == [[8]] and session.committed == [6]
  assert session.labels() == [list(range(21))]
  with pytest.raises(ValueError, match=r'horizon \+ chunk \+ 1 = 18'):
    session.push([np.zeros((9, 4))])
  plain = _session(1, 16)
  plain.push([np.zeros((14, 4))])
  plain.push([np.zeros((7, 4))])                  # horizon=None: nothing is automatic (the library refuses; the stand-in does not)
  assert not plain._decoder.horizons
  with pytest.raises(ValueError, match='horizon must be None or a non-negative integer'):
    host.OnlineSession(None, 1, None, 16, horizon=-2)


def test_the_symbols_are_declared_bound_and_exported():
  root = os.path.join(os.path.dirname(golden_util.GOLDEN_DIR), '..')
  header = open(os.path.join(root, 'include', 'uisrnn_hip.h')).read()
  assert 'int32_t uis_stream_commit(uis_handle* h, const int32_t* horizon, int32_t* labels_out, int64_t capacity,' in header
  assert 'int32_t uis_stream_committed(uis_handle* h, int64_t* committed_out);' in header
  for name in ('uis_stream_commit', 'uis_stream_committed'):
    assert name in _capi.EXPORTED_SYMBOLS
  lib = lib_build.OUTPUT
  if not os.path.exists(lib):
    lib = lib_build.build()
  symbols = subprocess.run(['nm', '-D', '--defined-only', lib], check=True, capture_output=True, text=True).stdout
  exported = {line.split()[-1] for line in symbols.splitlines() if line.strip()}
  assert {'uis_stream_commit', 'uis_stream_committed'} <= exported
