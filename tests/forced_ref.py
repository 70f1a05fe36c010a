"""CPU restatement of UISRNN.score_labels (uis_score_labels) for the tests.

The neg_likelihood of a fixed trace from an empty beam state (uisrnn/uisrnn.py:388-453, the
oracle's advance(), oracle/uis_oracle.c), written out frame by frame:
  - CoreRNN rows and the weighted MSE: the oracle's rnn_step / weighted_mse (include/uis_numerics.h);
  - priors in float64 in the oracle's expression order, with the C library's log (math.log);
  - the running mean, the step loss and the sum in numpy float32, one IEEE operation at a time.
"""

import math

import numpy as np

from oracle import oracle


def first_appearance(ids):
  """Ids of any hashable kind -> int32 labels by order of first appearance."""
  names = {}
  return np.array([names.setdefault(i, len(names)) for i in ids], dtype=np.int32)


def score_one(params, seq, labels):
  """(score float32, per-frame losses float32 [N]) of one utterance under `labels`.

  `labels` must be in first-appearance form except that a label larger than allowed makes the
  rest of the utterance +inf (the reference's invalid trace)."""
  x = np.asarray(seq, dtype=np.float32)
  n = x.shape[0]
  m0, h1 = oracle.constants(params)
  p0 = float(params['transition_bias'])
  alpha = float(params['crp_alpha'])
  lp_stay = math.log(1.0 - p0)
  lp_sw = math.log(p0)
  l_alpha = math.log(alpha)
  means, hids, counts, blk = [], [], [], []
  last, sumblk = -1, 0
  losses = np.full(n, np.inf, dtype=np.float32)
  score = np.float32(0.0)
  for t in range(n):
    c = int(labels[t])
    if c > len(means):
      return np.float32(np.inf), losses
    if c < len(means):
      mse = oracle.weighted_mse(params, means[c], x[t])
      if c == last:
        prior = lp_stay
      else:
        prior = lp_sw + math.log(float(blk[c])) - math.log(float(sumblk) + alpha)
      mean_out, hid = oracle.rnn_step(params, x[t], hids[c])
      k = counts[c]
      means[c] = (means[c] * np.float32(k - 1) + mean_out) / np.float32(k)  # three float32 ops per element
      hids[c] = hid
      counts[c] = k + 1
      if c != last:
        blk[c] += 1
        sumblk += 1
    else:
      mse = oracle.weighted_mse(params, m0, x[t])
      prior = lp_sw + l_alpha - math.log(float(sumblk) + alpha)
      mean_out, hid = oracle.rnn_step(params, x[t], h1)
      means.append(mean_out)
      hids.append(hid)
      counts.append(1)
      blk.append(1)
      sumblk += 1
    loss = np.float32(np.float64(mse) - prior)
    losses[t] = loss
    score = np.float32(score + loss)
    last = c
  return score, losses


def score(params, seqs, labels):
  """Scores and per-frame losses of a list of utterances."""
  out = [score_one(params, s, l) for s, l in zip(seqs, labels)]
  return np.array([o[0] for o in out], dtype=np.float32), [o[1] for o in out]
