"""CPU restatement of a session that retires clusters (uis_stream_retire) for the tests.

tests/commit_ref.py's Session -- primed_ref's beam search from a beam, with the commit rule -- plus the two
operations of include/uisrnn_hip.h's retirement and the id map of uisrnn_amd.OnlineSession:

  retirable()   the cluster indices k with, for every live hypothesis: k < K, k not among its labels of the window,
                k != its last label
  retire(R)     list surgery on every live primed_ref.Hypothesis: means / hids / counts / blk lose the entries in R,
                sumblk loses their block counts, last and the trace's labels become label - #{k in R : k < label}
                (the window's part of the trace; a committed frame that carried a retired cluster keeps no label)
  ids           index j of the present numbering is the j-th non-negative integer not in `gone`, the sorted retired
                ids: what the session hands out never changes and is never reused

Here `final`, labels() and what commit() returns are in stream ids; rows() stays in the present numbering (what
the library's n-best readout holds) and global_rows() maps it.  AutoSession adds model.online(..., retire_at=K)'s
rule, written from its description and not from the host code.
"""

import numpy as np

import commit_ref


def speaker_walk(seed, dim, n_speakers, segment, n_frames, noise=0.05, scale=1.0):
  """Frames around n_speakers unit centroids (times scale), `segment` frames each, one speaker after the other."""
  rng = np.random.default_rng(seed)
  cent = rng.standard_normal((n_speakers, dim))
  cent *= scale / np.linalg.norm(cent, axis=1, keepdims=True)
  ids = (np.arange(n_frames) // segment) % n_speakers
  return cent[ids] + noise * rng.standard_normal((n_frames, dim))


def to_global(j, gone):
  """The j-th non-negative integer that is not in the sorted list `gone` (negative j: no label, kept)."""
  if j < 0:
    return int(j)
  g = int(j)
  for x in gone:
    if x <= g:
      g += 1
    else:
      break
  return g


def to_local(g, gone):
  assert g not in gone
  return int(g) - sum(1 for x in gone if x < g)


def retire_hypothesis(hyp, R, committed):
  """`hyp` without the clusters in R (a new object; R ascending, every index below len(hyp.means))."""
  R = sorted(int(k) for k in R)
  drop = set(R)
  shift = lambda c: c - sum(1 for k in R if k < c)   # pylint: disable=unnecessary-lambda-assignment
  out = hyp.copy()
  keep = [k for k in range(len(hyp.means)) if k not in drop]
  out.means = [hyp.means[k] for k in keep]
  out.hids = [hyp.hids[k] for k in keep]
  out.counts = [hyp.counts[k] for k in keep]
  out.blk = [hyp.blk[k] for k in keep]
  out.sumblk = hyp.sumblk - sum(hyp.blk[k] for k in R)
  assert hyp.last not in drop
  out.last = shift(hyp.last) if hyp.last >= 0 else hyp.last
  out.trace = [(-1 if c in drop else shift(c)) if c >= 0 else c for c in hyp.trace[:committed]] + \
              [shift(c) for c in hyp.trace[committed:]]
  assert not drop & set(hyp.trace[committed:])
  return out


class Session(commit_ref.Session):
  """One utterance of a session that may retire clusters."""

  def __init__(self, params, beam_size, start=None):
    super().__init__(params, beam_size, start)
    self.gone = []        # the retired stream ids, sorted
    self.retired = []     # every retire() call's ids, in order

  def K(self):
    return max([len(h.means) for h in self.beam[:self.live]] or [0])

  def retirable(self):
    """Present indices, ascending."""
    if not self.live:
      return []
    beam = self.beam[:self.live]
    used = {int(c) for row in self.rows() for c in row} | {h.last for h in beam}
    return [k for k in range(min(len(h.means) for h in beam)) if k not in used]

  def retire(self, R):
    """R: present indices, every one retirable.  Returns their stream ids."""
    R = sorted(int(k) for k in R)
    assert len(set(R)) == len(R) and set(R) <= set(self.retirable()), (R, self.retirable())
    ids = [to_global(k, self.gone) for k in R]
    if R:
      self.beam = [retire_hypothesis(h, R, self.committed) for h in self.beam]
      self.gone = sorted(self.gone + ids)
    self.retired.append(ids)
    return ids

  def commit(self, horizon=None):
    n0 = len(self.final)
    out, dropped = super().commit(horizon)
    ids = [to_global(c, self.gone) for c in out]
    self.final[n0:] = ids
    return ids, dropped

  def global_rows(self):
    """The whole stream's labels of every live hypothesis in stream ids, committed part first."""
    return [list(self.final) + [to_global(int(c), self.gone) for c in row] for row in self.rows()]

  def labels(self):
    if not self.live:
      return list(self.final)
    return self.global_rows()[0]


class AutoSession(Session):
  """model.online(..., horizon=, retire_at=, retire_to=) for one utterance: before a push, when K at the last query
  plus the frames pushed since has reached retire_at: commit with the horizon, query, retire the retirable
  clusters, least recently seen in the committed labels first, until K <= retire_to."""

  def __init__(self, params, beam_size, horizon, retire_at, retire_to=None, start=None):
    super().__init__(params, beam_size, start)
    self.horizon, self.retire_at = horizon, int(retire_at)
    self.retire_to = int(retire_at) // 2 if retire_to is None else int(retire_to)
    self.bound = 0
    self.most = 0         # the largest K ever reached
    self.events = []      # (frames received, K before, ids retired)

  def push(self, chunk):
    chunk = np.asarray(chunk)
    if len(chunk) and self.bound >= self.retire_at:
      self.commit(self.horizon)
      seen = {c: t for t, c in enumerate(self.final)}
      k, able = self.K(), [to_global(j, self.gone) for j in self.retirable()]
      able.sort(key=lambda c: (seen.get(c, -1), c))
      pick = able[:max(k - self.retire_to, 0)]
      self.retire([to_local(c, self.gone) for c in pick])
      self.events.append((self.received, k, pick))
      self.bound = self.K()
    super().push(chunk)
    self.bound += len(chunk)
    self.most = max(self.most, self.K())
