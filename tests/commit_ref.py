"""CPU restatement of a session that commits (uis_stream_commit) for the tests.

The look_ahead-1 beam search of tests/primed_ref.py -- its Hypothesis, its Model and the candidate / sort rule
of its decode() -- started from a BEAM rather than from one hypothesis, one frame at a time, with the cut /
prune / commit rule of include/uisrnn_hip.h applied whenever the caller commits:

  have    frames in the window (received, not yet committed)
  stable  the leading window frames on which all live hypotheses agree (with test_iteration 1 two members
          of one beam never carry the same labels, so equal labels on [0, s) = one ancestor at step s - 1)
  cut     stable, or max(stable, have - horizon) with a horizon >= 0
  prune   (cut > stable) the hypotheses whose labels differ from rank 0's in [0, cut) leave; order, scores
          and state of the others stay
  commit  c = cut & ~1 labels of rank 0 are handed out, the window starts c frames later

A hypothesis keeps its whole trace here; the window is a view of it.  Every commit is recorded in
`history` (what the GPU tests assert their cases from: overlap of the move, non-contiguous survivors).
"""

import collections

import numpy as np

import nbest_ref
import primed_ref

Commit = collections.namedtuple('Commit', 'have stable cut committed kept dropped')


def step(model, beam, x, beam_size):
  """The beam after frame x: primed_ref.decode's loop body."""
  cand, scores, seen = [], [], {}
  for b, hyp in enumerate(beam):
    for c in range(len(hyp.means) + 1):
      cand.append((b, c))
      scores.append(hyp.candidate(model, x, c, seen))
  scores = np.array(scores, dtype=np.float32)
  finite = np.flatnonzero(np.isfinite(scores))
  order = finite[np.argsort(nbest_ref.score_key(scores[finite]), kind='stable')][:beam_size]
  return [beam[cand[i][0]].advance(model, x, cand[i][1], scores[i]) for i in order]


class Session:
  """One utterance of a session."""

  def __init__(self, params, beam_size, start=None):
    self.model = params if isinstance(params, primed_ref.Model) else primed_ref.Model(params)
    self.beam_size = int(beam_size)
    self.beam = [start if start is not None else primed_ref.Hypothesis()]
    self.received = len(self.beam[0].trace)
    self.committed = 0
    self.final = []       # the committed labels
    self.history = []     # a Commit per commit() call that found a live beam and a non-empty window

  @property
  def have(self):
    return self.received - self.committed

  @property
  def live(self):
    return len(self.beam) if self.received else 0   # (nothing received: the session has no hypothesis to show)

  def push(self, chunk):
    x = np.asarray(chunk, dtype=np.float32)
    for t in range(x.shape[0]):
      if self.beam:
        self.beam = step(self.model, self.beam, x[t], self.beam_size)
      self.received += 1

  def rows(self):
    """The window's labels of every live hypothesis, best first: int32 [live, have]."""
    if not self.live:
      return np.zeros((0, self.have), dtype=np.int32)
    return np.array([h.trace[self.committed:] for h in self.beam], dtype=np.int32).reshape(len(self.beam), self.have)

  def scores(self):
    return np.array([h.score for h in self.beam[:self.live]], dtype=np.float32)

  def stable(self):
    return nbest_ref.common_prefix(self.rows()) if self.live else 0

  def labels(self):
    """Everything received under the best hypothesis: committed part first."""
    return list(self.beam[0].trace) if self.live else list(self.final)

  def commit(self, horizon=None):
    """Returns (labels that became final, hypotheses dropped)."""
    have = self.have
    if have == 0 or not self.live:
      return [], 0
    rows = self.rows()
    stable = nbest_ref.common_prefix(rows)
    cut = stable
    if horizon is not None and horizon >= 0:
      cut = max(stable, have - int(horizon))
    kept = list(range(len(self.beam)))
    if cut > stable:
      kept = [k for k in kept if np.array_equal(rows[k][:cut], rows[0][:cut])]
    dropped = len(self.beam) - len(kept)
    self.beam = [self.beam[k] for k in kept]
    c = cut & ~1
    out = [int(v) for v in rows[0][:c]]
    self.final.extend(out)
    self.committed += c
    self.history.append(Commit(have, stable, cut, c, kept, dropped))
    return out, dropped


class ReplaySession:
  """Session without a horizon, read off nbest_ref.replay (the oracle's own candidate scores, in C) instead of
  running the beam search in Python: a commit without a horizon prunes nothing, so the beam after t frames is the
  replay's.  Same readouts and the same commit rule; tests/test_commit_host.py holds it against Session."""

  def __init__(self, rep):
    self.rep = rep
    self.received = 0
    self.committed = 0
    self.final = []
    self.history = []

  @property
  def have(self):
    return self.received - self.committed

  def push(self, n):
    self.received += int(n)
    assert self.received <= self.rep.n_frames

  def full_rows(self):
    return nbest_ref.nbest(self.rep, upto=self.received)

  def commit(self, horizon=None):
    assert horizon is None
    rows = self.full_rows()[0][:, self.committed:]
    if self.have == 0 or rows.shape[0] == 0:
      return [], 0
    stable = nbest_ref.common_prefix(rows)
    c = stable & ~1
    out = [int(v) for v in rows[0][:c]]
    self.history.append(Commit(self.have, stable, stable, c, list(range(rows.shape[0])), 0))
    self.final.extend(out)
    self.committed += c
    return out, 0


def run(params, seq, beam_size, chunk, horizon=None, commit=True, auto_window=None):
  """One utterance pushed in chunks of `chunk` frames.

  commit=True: commit(horizon) after every push.  auto_window=W: model.online(..., max_frames=W, horizon=...)'s
  rule instead -- commit only when the next chunk does not fit the window.
  Returns (session, snapshots): after every push, before its commit, dict(labels, rows, scores, stable,
  committed)."""
  session = Session(params, beam_size)
  shots = []
  n = seq.shape[0]
  for t0 in range(0, n, chunk):
    part = seq[t0:t0 + chunk]
    if auto_window is not None and session.have + len(part) > auto_window:
      session.commit(horizon)
      assert session.have + len(part) <= auto_window, (session.have, len(part), auto_window)
    session.push(part)
    shots.append({'labels': session.labels(), 'rows': session.rows(), 'scores': session.scores(),
                  'stable': session.committed + session.stable(), 'committed': session.committed})
    if auto_window is None and commit:
      session.commit(horizon)
  return session, shots
