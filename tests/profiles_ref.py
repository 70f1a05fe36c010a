"""CPU restatement of uis_speaker_profiles for the tests.

Along a given labeling, per cluster: frames, blocks, first and last frame, the running mean after its last frame, the
float32 sum of its frames and the float32 sum of squared residuals against the mean each frame was charged against.
  - CoreRNN rows: the oracle's rnn_step (include/uis_numerics.h);
  - the running mean: the line of speakers_ref.rows_one, three float32 operations per element;
  - the residual step: r = x - P, acc = acc + r * r, and sum_x = sum_x + x, numpy float32, one IEEE operation at a time.
"""

import numpy as np

import forced_ref
import speakers_ref
from oracle import oracle


class Profile(object):
  """One utterance: n_clusters (-1: an invalid trace), stats int32 [K, 4] {n, blocks, first, last}, mean / sum_x /
  sum_r2 float32 [K, D], priors: the mean rows P_j each frame was charged against, float32 [N, D] (the float64 check
  takes them as inputs), score float32."""

  def __init__(self, n_clusters, stats, mean, sum_x, sum_r2, priors, score):
    self.n_clusters, self.stats, self.mean, self.sum_x, self.sum_r2 = n_clusters, stats, mean, sum_x, sum_r2
    self.priors, self.score = priors, score


def profile_one(params, seq, labels, want_score=True):
  x = np.asarray(seq, dtype=np.float32)
  n, dim = x.shape[0], int(params['observation_dim'])
  labels = np.asarray(labels, dtype=np.int32)
  m0, h1 = oracle.constants(params)
  m0 = np.asarray(m0, dtype=np.float32)
  score = forced_ref.score_one(params, x, labels)[0] if want_score else None
  if speakers_ref.cluster_count(labels) != (int(labels.max()) + 1 if n else 0):
    return Profile(-1, np.zeros((0, 4), np.int32), np.zeros((0, dim), np.float32), np.zeros((0, dim), np.float32),
                   np.zeros((0, dim), np.float32), np.zeros((0, dim), np.float32), score)
  means, hids, counts, stats, sum_x, sum_r2 = [], [], [], [], [], []
  priors = np.zeros((n, dim), dtype=np.float32)
  last = -1
  for t in range(n):
    c = int(labels[t])
    if c == len(means):
      means.append(None)
      hids.append(h1)
      counts.append(0)
      stats.append([0, 0, t, t])
      sum_x.append(np.zeros(dim, dtype=np.float32))
      sum_r2.append(np.zeros(dim, dtype=np.float32))
    prior = m0 if means[c] is None else means[c]
    priors[t] = prior
    with np.errstate(all='ignore'):
      r = (x[t] - prior).astype(np.float32)
      sum_r2[c] = (sum_r2[c] + (r * r).astype(np.float32)).astype(np.float32)
      sum_x[c] = (sum_x[c] + x[t]).astype(np.float32)
      mean_out, hid = oracle.rnn_step(params, x[t], hids[c])
      k = counts[c]
      if k == 0:
        means[c] = np.asarray(mean_out, dtype=np.float32).copy()
      else:
        means[c] = (means[c] * np.float32(k - 1) + mean_out) / np.float32(k)  # speakers_ref.rows_one's line, k = frames so far
    hids[c] = hid
    counts[c] = k + 1
    stats[c][0] += 1
    stats[c][3] = t
    if c != last:
      stats[c][1] += 1
    last = c
  arr = lambda rows: np.array(rows, dtype=np.float32).reshape(len(means), dim)
  return Profile(len(means), np.array(stats, dtype=np.int32).reshape(len(means), 4), arr(means), arr(sum_x), arr(sum_r2),
                 priors, score)


def profiles(params, seqs, labels, want_score=True):
  return [profile_one(params, s, l, want_score) for s, l in zip(seqs, labels)]


def padded(profs, width, dim):
  """The call's arrays from a list of Profile: n_clusters [U], stats [U, width, 4], mean / sum_x / sum_r2 [U, width, D],
  absent rows {0, 0, -1, -1} and +0.0."""
  n_utt = len(profs)
  out = {'n_clusters': np.array([p.n_clusters for p in profs], dtype=np.int32),
         'stats': np.tile(np.array([0, 0, -1, -1], dtype=np.int32), (n_utt, width, 1)),
         'mean': np.zeros((n_utt, width, dim), np.float32), 'sum_x': np.zeros((n_utt, width, dim), np.float32),
         'sum_r2': np.zeros((n_utt, width, dim), np.float32)}
  for u, p in enumerate(profs):
    k = max(p.n_clusters, 0)
    out['stats'][u, :k] = p.stats
    for key in ('mean', 'sum_x', 'sum_r2'):
      out[key][u, :k] = getattr(p, key)
  return out


def stats_numpy(labels):
  """{n, blocks, first, last} per cluster, from numpy on the labels alone."""
  labels = np.asarray(labels, dtype=np.int64)
  k = int(labels.max()) + 1 if labels.size else 0
  starts = np.flatnonzero(np.concatenate([[True], labels[1:] != labels[:-1]])) if labels.size else np.zeros(0, np.int64)
  out = np.zeros((k, 4), dtype=np.int32)
  for c in range(k):
    at = np.flatnonzero(labels == c)
    out[c] = [at.size, int(np.sum(labels[starts] == c)), at[0], at[-1]]
  return out
