"""CPU restatement of the n-best readout for the tests: the whole beam history of one utterance.

oracle.decode hands out rank 0's labels and the final beam's scores only.  Here the history of every
rank is rebuilt from oracle.candidate_scores -- every candidate score of every window, dense
[windows, B] + [cmax] * L -- by doing the prune again in numpy: per window the candidates are
flattened [B, cmax ** L] row-major (hypothesis, then the assignment tuple: the oracle's enumeration
order) and sorted stably by uis_score_key (include/uis_numerics.h), which is the oracle's cand_cmp;
the leading finite ones, at most B, are the next beam; parent = index // cmax ** L and the path is
the index's digits in base cmax.  Tracing every final rank back gives every hypothesis' labels.

With test_iteration 1 and look_ahead 1 window w is step w and depends on frames 0 .. w only, so one
replay serves every prefix length of a streamed utterance (`upto`).
"""

import collections

import numpy as np

from oracle import oracle

Replay = collections.namedtuple('Replay', 'parents paths scores n_frames look_ahead test_iteration')


def score_key(scores):
  """uis_score_key on a float32 array: ascending key = ascending value, -0 == +0."""
  s = np.array(scores, dtype=np.float32)
  s[s == 0.0] = 0.0
  u = s.view(np.uint32)
  return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def replay(params, seq, beam_size, look_ahead=1, test_iteration=1):
  """The beam after every window: parents[w] int [width_w], paths[w] int [width_w, L] (-1 past a
  ragged last window), scores[w] float32 [width_w]."""
  n = int(seq.shape[0])
  total = test_iteration * n
  n_win = (total + look_ahead - 1) // look_ahead
  cmax = 4
  while True:
    grid = oracle.candidate_scores(params, seq, beam_size, look_ahead, test_iteration, cmax)
    stride = cmax ** look_ahead
    parents, paths, scores = [], [], []
    clusters = np.zeros(1, dtype=np.int64)  # K of every hypothesis of the current beam
    fits = True
    for w in range(n_win):
      # a hypothesis with K clusters has candidates 0 .. K at the window's first frame, up to K + L - 1 at its last
      if clusters.size and int(clusters.max()) + look_ahead > cmax:
        fits = False
        break
      lw = min(look_ahead, total - w * look_ahead)
      flat = grid[w].reshape(-1)
      order = np.argsort(score_key(flat), kind='stable')
      finite = np.isfinite(flat[order])
      n_fin = int(finite.size if finite.all() else np.argmin(finite))  # non-finite sort last; a leading one ends it
      keep = order[:min(n_fin, beam_size)]
      par = keep // stride
      digits = np.empty((keep.size, look_ahead), dtype=np.int64)
      rest = keep % stride
      for j in range(look_ahead - 1, -1, -1):
        digits[:, j] = rest % cmax
        rest = rest // cmax
      digits[:, lw:] = -1
      parents.append(par)
      paths.append(digits)
      scores.append(flat[keep].astype(np.float32))
      clusters = np.maximum(clusters[par], digits.max(axis=1) + 1) if keep.size else np.zeros(0, dtype=np.int64)
    if fits:
      return Replay(parents, paths, scores, n, look_ahead, test_iteration)
    cmax *= 2


def nbest(rep, upto=None):
  """(rows int32 [width, N], scores float32 [width]): trace[-N:] of every hypothesis of the final
  beam, best first.  upto (test_iteration 1, look_ahead 1 only): the beam after the first `upto`
  frames instead."""
  n = rep.n_frames
  n_win = len(rep.parents)
  if upto is not None:
    assert rep.look_ahead == 1 and rep.test_iteration == 1
    n = n_win = int(upto)
  if n_win == 0:
    return np.zeros((0, n), dtype=np.int32), np.zeros(0, dtype=np.float32)
  width = rep.parents[n_win - 1].size
  rows = np.empty((width, n), dtype=np.int32)
  for k in range(width):
    labels = []
    r = k
    for w in range(n_win - 1, -1, -1):
      path = [int(c) for c in rep.paths[w][r] if c >= 0]
      labels[:0] = path
      r = int(rep.parents[w][r])
    rows[k] = labels[len(labels) - n:] if n else []
  return rows, rep.scores[n_win - 1].copy()


def common_prefix(rows):
  """The number of leading columns on which all rows agree (0 rows: 0)."""
  if rows.shape[0] == 0:
    return 0
  same = (rows == rows[0]).all(axis=0)
  return int(same.size if same.all() else np.argmin(same))
