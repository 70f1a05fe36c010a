"""Session restarts' CPU side: the symbol, the refusals that need no device, and the Python layer's bookkeeping
(OnlineSession.restart, StreamPool) against a stand-in decoder.  No GPU needed.
"""

import ctypes
import os
import subprocess

import numpy as np
import pytest

import golden_util
import uisrnn_amd
from uisrnn_amd import _capi
from uisrnn_amd import build as lib_build
from uisrnn_amd import uisrnn as host

_i32p = ctypes.POINTER(ctypes.c_int32)


def test_the_symbol_is_declared_bound_and_exported():
  root = os.path.join(os.path.dirname(golden_util.GOLDEN_DIR), '..')
  header = open(os.path.join(root, 'include', 'uisrnn_hip.h')).read()
  assert ('int32_t uis_stream_restart(uis_handle* h, const int32_t* which, int32_t* labels_out, int64_t capacity,\n'
          '                           int32_t* counts_out, float* scores_out, int32_t* overflow_out);') in header
  assert 'uis_stream_restart' in _capi.EXPORTED_SYMBOLS
  lib = lib_build.OUTPUT
  if not os.path.exists(lib):
    lib = lib_build.build()
  symbols = subprocess.run(['nm', '-D', '--defined-only', lib], check=True, capture_output=True, text=True).stdout
  assert 'uis_stream_restart' in {line.split()[-1] for line in symbols.splitlines() if line.strip()}
  assert hasattr(_capi.Decoder, 'stream_restart') and hasattr(host.OnlineSession, 'restart')
  assert uisrnn_amd.StreamPool is host.StreamPool and hasattr(uisrnn_amd.UISRNN, 'online_pool')


def test_without_a_handle_the_call_refuses_and_writes_nothing():
  lib = _capi.load_library()
  which = np.ones(2, dtype=np.int32)
  counts = np.full(2, -7, dtype=np.int32)
  labels = np.full(4, -7, dtype=np.int32)
  scores = np.full(2, -7.0, dtype=np.float32)
  rc = lib.uis_stream_restart(None, which.ctypes.data_as(_i32p), labels.ctypes.data_as(_i32p), 4,
                              counts.ctypes.data_as(_i32p), scores.ctypes.data_as(_capi._fp), None)   # pylint: disable=protected-access
  assert rc == _capi.UIS_ERR_INVALID_ARG
  assert 'null handle' in _capi.last_error(lib)
  assert (counts == -7).all() and (labels == -7).all() and (scores == -7.0).all()


class _StandIn:
  """A decoder that records what reaches it (no library, no device): a window of `have` frames whose labels are
  their own positions in the stream, scores = frames received; `dead` utterances report the overflow word."""

  def __init__(self, n_utt):
    self.have = np.zeros(n_utt, dtype=np.int64)
    self.done = np.zeros(n_utt, dtype=np.int64)
    self.dead = set()
    self.empty_beam = set()
    self.restarts = []
    self.closed = False

  def stream_received(self):
    return self.have.copy()

  def stream_committed(self):
    return self.done.copy()

  def stream_push(self, chunks):
    for u, c in enumerate(chunks):
      self.have[u] += 0 if c is None else len(c)

  def stream_prime(self, chunks, labels):
    for u, lab in enumerate(labels):
      self.have[u] += 0 if lab is None else len(lab)
    return np.zeros(len(self.have), dtype=np.float32)

  def stream_commit(self, horizon):
    out = []
    for u in range(len(self.have)):
      cut = 0 if horizon is None or horizon[u] < 0 else max(int(self.have[u]) - horizon[u], 0)
      c = cut & ~1
      out.append(np.arange(self.done[u], self.done[u] + c, dtype=np.int32))
      self.done[u] += c
      self.have[u] -= c
    return out, np.zeros(len(self.have), dtype=np.int32)

  def _window(self, u):
    if u in self.empty_beam:
      return np.full(self.have[u], -1, dtype=np.int32)
    return np.arange(self.done[u], self.done[u] + self.have[u], dtype=np.int32)

  def stream_labels(self):
    overflow = np.array([1 if u in self.dead else 0 for u in range(len(self.have))], dtype=np.int32)
    return [self._window(u) for u in range(len(self.have))], None, overflow, 0

  def stream_restart(self, which):
    self.restarts.append(list(which))
    n_utt = len(self.have)
    labels = [self._window(u) if which[u] else np.zeros(0, dtype=np.int32) for u in range(n_utt)]
    scores = np.array([float(self.done[u] + self.have[u]) if which[u] else np.nan for u in range(n_utt)], dtype=np.float32)
    overflow = np.array([1 if which[u] and u in self.dead else 0 for u in range(n_utt)], dtype=np.int32)
    for u in range(n_utt):
      if which[u]:
        self.have[u] = self.done[u] = 0
        self.dead.discard(u)
        self.empty_beam.discard(u)
    return labels, scores, overflow, _capi.UIS_ERR_CLUSTER_CAP if overflow.any() else 0

  def stream_end(self):
    self.closed = True

  def close(self):
    self.closed = True


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
  session._open = True
  return session


def test_restart_hands_out_the_whole_stream_and_forgets_it():
  session = _session(3, 100)
  session.push([np.zeros((9, 4)), np.zeros((4, 4)), np.zeros((6, 4))])
  assert session.commit([3, None, 0]) == [[0, 1, 2, 3, 4, 5], [], [0, 1, 2, 3, 4, 5]]
  assert session.committed == [6, 0, 6]
  out = session.restart([2, 0])
  assert out == [(list(range(9)), 9.0), None, (list(range(6)), 6.0)]     # committed labels first, then the window's
  assert session._decoder.restarts == [[1, 0, 1]]
  assert session._final == [[], [], []] and session.committed == [0, 0, 0]
  assert session.labels() == [[], list(range(4)), []]
  # the slot is new: it can be primed, pushed and committed again
  session.prime([np.zeros((2, 4)), None, None], [[0, 0], None, None])
  session.push([np.zeros((3, 4)), None, np.zeros((2, 4))])
  assert session.labels() == [list(range(5)), list(range(4)), [0, 1]]
  with pytest.raises(ValueError, match='already received 4 frames'):      # the neighbour is not
    session.prime([None, np.zeros((2, 4)), None], [None, [0, 0], None])
  assert session.restart([]) == [None, None, None] and session._decoder.restarts[-1] == [0, 0, 0]
  assert session.restart(iter([np.int64(1)]))[1] == (list(range(4)), 4.0)


def test_restart_argument_errors_touch_nothing():
  session = _session(3, 100)
  session.push([np.zeros((5, 4))] * 3)
  for bad, match in (([3], 'not in'), ([-1], 'not in'), ([1, 1], 'given twice'), ([True], 'not in'), ([0.0], 'not in'),
                     (['0'], 'not in')):
    with pytest.raises(ValueError, match=match):
      session.restart(bad)
  assert not session._decoder.restarts and session.labels() == [list(range(5))] * 3


def test_restart_does_not_raise_for_a_dead_slot():
  session = _session(3, 100)
  session.push([np.zeros((5, 4))] * 3)
  session._decoder.dead.add(1)
  session._decoder.empty_beam.add(2)
  with pytest.raises(RuntimeError, match='max_clusters'):
    session.labels()
  out = session.restart([0, 1, 2])
  assert out == [(list(range(5)), 5.0), (None, 5.0), (None, 5.0)]
  assert session.labels() == [[], [], []]


def test_the_automatic_commit_keeps_working_after_a_restart():
  session = _session(1, 16, horizon=8)
  for _ in range(3):
    session.push([np.zeros((7, 4))])           # the third push commits 6 first
  assert session.committed == [6]
  assert session.restart([0])[0] == (list(range(21)), 21.0)
  for _ in range(3):
    session.push([np.zeros((7, 4))])
  assert session.committed == [6] and session.labels() == [list(range(21))]


def test_stream_pool_bookkeeping():
  session = _session(2, 100)
  pool = host.StreamPool(session)
  assert pool.open('a') == 0 and pool.open('b') == 1
  with pytest.raises(RuntimeError, match='no free slot'):
    pool.open('c')
  with pytest.raises(KeyError):
    pool.open('a')
  pool.push({'b': np.zeros((3, 4))})
  pool.push({'a': np.zeros((2, 4)), 'b': np.zeros((1, 4))})
  assert pool.labels('a') == [0, 1] and pool.labels('b') == [0, 1, 2, 3]
  with pytest.raises(KeyError):
    pool.push({'c': np.zeros((1, 4))})
  with pytest.raises(KeyError):
    pool.finish('c')
  assert pool.finish('b') == ([0, 1, 2, 3], 4.0)
  with pytest.raises(KeyError):
    pool.labels('b')
  assert pool.open('c') == 1                     # the slot that was freed
  pool.push({'c': np.zeros((1, 4))})
  assert pool.labels('c') == [0] and pool.labels('a') == [0, 1]
  assert pool.finish('a') == ([0, 1], 2.0) and pool.finish('c') == ([0], 1.0)
  assert pool.open('d') in (0, 1)
  with pool:
    pass
  assert session._decoder.closed
