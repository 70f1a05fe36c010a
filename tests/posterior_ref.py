"""CPU restatement of the posterior readout for the tests, in float64.

Inputs are (rows, scores) as tests/nbest_ref.py's replay of the oracle gives them -- the device's n-best readout
equals that replay bit for bit (tests/test_gpu_nbest.py), so nothing here depends on the code under test:
  w_k           = exp(-(s_k - s_0) / temperature) / Z,  Z = sum_j exp(-(s_j - s_0) / temperature)
  confidence[t] = sum_k w_k [lab_k[t] == lab_0[t]]
  change[t]     = sum_k w_k [lab_k[t] != lab_k[t - 1]]  for t >= 1, change[0] = 0
No live hypothesis: zeros.
"""

import numpy as np


def posterior(rows, scores, temperature):
  """(confidence float64 [N], change float64 [N], weights float64 [live]) of rows int [live, N] and their float32
  scores, ascending."""
  rows = np.asarray(rows)
  live, n = rows.shape
  if live == 0:
    return np.zeros(n), np.zeros(n), np.zeros(0)
  s = np.asarray(scores, dtype=np.float32).astype(np.float64)
  assert s.shape == (live,)
  e = np.exp(-(s - s[0]) / float(temperature))
  w = e / e.sum()
  confidence = (w[:, None] * (rows == rows[0])).sum(axis=0)
  change = np.zeros(n)
  if n > 1:
    change[1:] = (w[:, None] * (rows[:, 1:] != rows[:, :-1])).sum(axis=0)
  return confidence, change, w


def tolerance(live):
  """|device - reference| allowed, absolute, for confidence, change and the weights.  Every term is in [0, 1]; each
  weight carries a few float32 roundings (the subtraction, the division by the temperature, expf at <= 1 ulp), each
  of the <= live additions of numerator and denominator one rounding of a partial sum <= 1, and the quotient doubles
  that."""
  return (live + 8) * 2.0 ** -23


def interior(values):
  """Some entry lies strictly inside (0.001, 0.999): weighting matters for it."""
  values = np.asarray(values)
  return bool(((values > 0.001) & (values < 0.999)).any())
