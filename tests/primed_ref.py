"""CPU restatement of a primed online decode (uis_stream_prime + pushes) for the tests.

A hypothesis is what _update_beam_state (uisrnn/uisrnn.py:388-453) keeps: per cluster the running mean, the
hidden state, the frame count and the block count, the last label, sum(block_counts), the float32
neg_likelihood and the trace.  advance() is tests/forced_ref.py's score_one loop, one frame at a time and
keeping the state; advance_forced() runs it along given labels (the prefix); decode() is the look_ahead-1
beam search over it, from whatever hypothesis it is given.

Built only from oracle.rnn_step, oracle.weighted_mse and oracle.constants:
  - priors in float64 in the oracle's expression order, with the C library's log (math.log);
  - the running mean, the step loss and the sum in numpy float32, one IEEE operation at a time;
  - a step's candidates are 0 .. K of every live hypothesis, in (hypothesis, cluster) order; their scores
    float32(score + float32(float64(mse) - prior)); the finite ones are sorted stably by
    nbest_ref.score_key and the leading min(#finite, beam_size) are the next beam.
With an empty prefix this is oracle.decode(params, seqs, beam, 1, 1) bit for bit (tests/test_prime_host.py),
which is what makes it a reference.
"""

import math

import numpy as np

import nbest_ref
from oracle import oracle


class Model:
  """The per-model constants every hypothesis shares."""

  def __init__(self, params):
    # (the weights as float32 once: the oracle's wrappers cast whatever they are given at every call)
    self.params = {k: [np.ascontiguousarray(a, dtype=np.float32) for a in v] if isinstance(v, list) else
                      np.ascontiguousarray(v, dtype=np.float32) if isinstance(v, np.ndarray) else v
                   for k, v in params.items()}
    params = self.params
    self.m0, self.h1 = oracle.constants(params)
    p0 = float(params['transition_bias'])
    self.alpha = float(params['crp_alpha'])
    self.lp_stay = math.log(1.0 - p0)
    self.lp_sw = math.log(p0)
    self.l_alpha = math.log(self.alpha)


class Hypothesis:
  """One BeamState plus its cluster states."""

  def __init__(self):
    self.means, self.hids, self.counts, self.blk = [], [], [], []
    self.last, self.sumblk = -1, 0
    self.score = np.float32(0.0)
    self.trace = []

  def copy(self):
    h = Hypothesis()
    h.means, h.hids = list(self.means), list(self.hids)  # (entries are replaced, never written into)
    h.counts, h.blk = list(self.counts), list(self.blk)
    h.last, h.sumblk, h.score, h.trace = self.last, self.sumblk, self.score, list(self.trace)
    return h

  def candidate(self, model, x, c, seen=None):
    """float32 score of this hypothesis with frame x given to cluster c (0 .. K).  seen: the MSEs of this frame
    against cluster states already met (hypotheses share them; keyed by the mean array's identity)."""
    seen = {} if seen is None else seen
    mean = self.means[c] if c < len(self.means) else model.m0
    if id(mean) not in seen:
      seen[id(mean)] = oracle.weighted_mse(model.params, mean, x)
    mse = seen[id(mean)]
    if c < len(self.means):
      if c == self.last:
        prior = model.lp_stay
      else:
        prior = model.lp_sw + math.log(float(self.blk[c])) - math.log(float(self.sumblk) + model.alpha)
    else:
      prior = model.lp_sw + model.l_alpha - math.log(float(self.sumblk) + model.alpha)
    loss = np.float32(np.float64(mse) - prior)
    return np.float32(self.score + loss)

  def advance(self, model, x, c, score=None):
    """The hypothesis after frame x went to cluster c (a new object)."""
    h = self.copy()
    h.score = self.candidate(model, x, c) if score is None else np.float32(score)
    if c < len(self.means):
      mean_out, hid = oracle.rnn_step(model.params, x, self.hids[c])
      k = self.counts[c]
      h.means[c] = (self.means[c] * np.float32(k - 1) + mean_out) / np.float32(k)  # three float32 ops per element
      h.hids[c] = hid
      h.counts[c] = k + 1
      if c != self.last:
        h.blk[c] += 1
        h.sumblk += 1
    else:
      mean_out, hid = oracle.rnn_step(model.params, x, model.h1)
      h.means.append(mean_out)
      h.hids.append(hid)
      h.counts.append(1)
      h.blk.append(1)
      h.sumblk += 1
    h.last = c
    h.trace.append(c)
    return h


def advance_forced(model, seq, labels, start=None):
  """The hypothesis after `labels` (first-appearance form) along the float32 frames of `seq`."""
  x = np.asarray(seq, dtype=np.float32)
  hyp = start if start is not None else Hypothesis()
  for t in range(len(labels)):
    c = int(labels[t])
    assert 0 <= c <= len(hyp.means), 'not in first-appearance form'
    hyp = hyp.advance(model, x[t], c)
  return hyp


def decode(model, seq, beam_size, start=None):
  """look_ahead-1 beam search over the frames of `seq` from the beam [start] (default: an empty hypothesis).

  Returns the final beam, best first (a list of Hypothesis; empty when every candidate of a step was
  non-finite)."""
  x = np.asarray(seq, dtype=np.float32)
  beam = [start if start is not None else Hypothesis()]
  for t in range(x.shape[0]):
    cand, scores, seen = [], [], {}
    for b, hyp in enumerate(beam):
      for c in range(len(hyp.means) + 1):
        cand.append((b, c))
        scores.append(hyp.candidate(model, x[t], c, seen))
    scores = np.array(scores, dtype=np.float32)
    finite = np.flatnonzero(np.isfinite(scores))
    order = finite[np.argsort(nbest_ref.score_key(scores[finite]), kind='stable')][:beam_size]
    beam = [beam[cand[i][0]].advance(model, x[t], cand[i][1], scores[i]) for i in order]
    if not beam:
      break
  return beam


def primed_decode(params, seq, prefix_labels, beam_size):
  """Prime with prefix_labels over seq[:P], beam-search the rest.

  Returns dict(labels int32 [width, N] best first, scores float32 [width], prefix_score float32)."""
  model = Model(params)
  p = len(prefix_labels)
  start = advance_forced(model, seq[:p], prefix_labels)
  beam = decode(model, seq[p:], beam_size, start) if seq.shape[0] > p else [start]
  n = seq.shape[0]
  return {'labels': np.array([h.trace for h in beam], dtype=np.int32).reshape(len(beam), n),
          'scores': np.array([h.score for h in beam], dtype=np.float32),
          'prefix_score': np.float32(start.score)}


def padded_beam(scores, beam_size):
  """The final beam's scores as uis_last_decode_info hands them out: +inf padded to beam_size."""
  out = np.full(beam_size, np.inf, dtype=np.float32)
  out[:len(scores)] = scores
  return out
