"""CPU restatement of UISRNN.score_speakers (uis_score_speakers) for the tests.

forced_ref.score_one extended from the chosen column to the whole row: at frame t, the step loss of assigning the
frame to every cluster open so far and to a new one, given the labeled history before t -- the row _calculate_score
(uisrnn/uisrnn.py:455-477) forms for that hypothesis:
  - CoreRNN rows and the weighted MSE: the oracle's rnn_step / weighted_mse (include/uis_numerics.h);
  - priors in float64 in the oracle's expression order, with the C library's log (math.log);
  - the running mean, the step loss and the sum in numpy float32, one IEEE operation at a time.
"""

import math

import numpy as np

from oracle import oracle


def cluster_count(labels):
  """Clusters of the valid trace: an invalid label (past first-appearance form) ends it."""
  k = 0
  for c in labels:
    if int(c) > k:
      break
    if int(c) == k:
      k += 1
  return k


def _mse_only(params):
  """A one-unit model with `params`' observation_dim and sigma2.  oracle.weighted_mse reads nothing else of a model
  but prepares all of it on every call, and a row needs one call per open cluster: this keeps a call cheap."""
  dim = int(params['observation_dim'])
  zeros = lambda *shape: np.zeros(shape, dtype=np.float32)
  return {'observation_dim': dim, 'rnn_hidden_size': 1, 'rnn_depth': 1,
          'gru_weight_ih': [zeros(3, dim)], 'gru_weight_hh': [zeros(3, 1)], 'gru_bias_ih': [zeros(3)],
          'gru_bias_hh': [zeros(3)], 'linear_mean1_weight': zeros(1, 1), 'linear_mean1_bias': zeros(1),
          'linear_mean2_weight': zeros(dim, 1), 'linear_mean2_bias': zeros(dim), 'rnn_init_hidden': zeros(1, 1),
          'sigma2': params['sigma2'], 'transition_bias': params['transition_bias'], 'crp_alpha': params['crp_alpha']}


def rows_one(params, seq, labels, width=None):
  """(score float32, rows float32 [N, width]) of one utterance under `labels`; width defaults to clusters + 1.

  rows[t, k]: k < K(t) the loss of staying with / returning to cluster k, k == K(t) of opening a new one, +inf past
  it; every row from the first label larger than allowed on is all +inf (the reference's invalid trace)."""
  x = np.asarray(seq, dtype=np.float32)
  n = x.shape[0]
  if width is None:
    width = cluster_count(labels) + 1
  m0, h1 = oracle.constants(params)
  mse_params = _mse_only(params)
  p0 = float(params['transition_bias'])
  alpha = float(params['crp_alpha'])
  lp_stay = math.log(1.0 - p0)
  lp_sw = math.log(p0)
  l_alpha = math.log(alpha)
  means, hids, counts, blk = [], [], [], []
  last, sumblk = -1, 0
  rows = np.full((n, width), np.inf, dtype=np.float32)
  score = np.float32(0.0)
  for t in range(n):
    c = int(labels[t])
    if c > len(means):
      return np.float32(np.inf), rows
    logden = math.log(float(sumblk) + alpha)
    for k in range(len(means)):
      mse = oracle.weighted_mse(mse_params, means[k], x[t])
      prior = lp_stay if k == last else lp_sw + math.log(float(blk[k])) - logden
      rows[t, k] = np.float32(np.float64(mse) - prior)
    mse = oracle.weighted_mse(mse_params, m0, x[t])
    rows[t, len(means)] = np.float32(np.float64(mse) - (lp_sw + l_alpha - logden))
    if c < len(means):
      mean_out, hid = oracle.rnn_step(params, x[t], hids[c])
      k = counts[c]
      means[c] = (means[c] * np.float32(k - 1) + mean_out) / np.float32(k)  # three float32 ops per element
      hids[c] = hid
      counts[c] = k + 1
      if c != last:
        blk[c] += 1
        sumblk += 1
    else:
      mean_out, hid = oracle.rnn_step(params, x[t], h1)
      means.append(mean_out)
      hids.append(hid)
      counts.append(1)
      blk.append(1)
      sumblk += 1
    score = np.float32(score + rows[t, c])
    last = c
  return score, rows


def rows(params, seqs, labels, width=None):
  """Scores [U] and the rows of a list of utterances, each [N_u, width] (None: its own clusters + 1)."""
  out = [rows_one(params, s, l, width) for s, l in zip(seqs, labels)]
  return np.array([o[0] for o in out], dtype=np.float32), [o[1] for o in out]


def candidates(rows_u, labels):
  """float32(cum_{t-1} + rows[t]) with cum_t = float32(cum_{t-1} + rows[t, c_t]), cum_{-1} = 0: the candidate scores
  of the one hypothesis a beam-1 decode carries along `labels`."""
  out = np.empty_like(rows_u)
  cum = np.float32(0.0)
  for t in range(rows_u.shape[0]):
    out[t] = (cum + rows_u[t]).astype(np.float32)
    cum = np.float32(cum + rows_u[t, int(labels[t])])
  return out


# ---- the hand-made labelings of the tests

def revisiting(n, clusters=18):
  """Cluster j opens at frame 2 j; every other frame goes back to cluster (7 t) mod K(t)."""
  out, k = [], 0
  for t in range(n):
    if t % 2 == 0 and k < clusters:
      out.append(k)
      k += 1
    else:
      out.append((t * 7) % k)
  return np.array(out, dtype=np.int32)


def one_cluster(n):
  return np.zeros(n, dtype=np.int32)


def all_new(n):
  return np.arange(n, dtype=np.int32)


def invalid_at(n, at=20):
  """Three speakers in turns of four frames, with K + 1 written at frame `at`: rows `at` and later are +inf."""
  out = (np.arange(n, dtype=np.int32) // 4) % 3
  k = cluster_count(out[:at])
  out[at] = k + 1
  return out
