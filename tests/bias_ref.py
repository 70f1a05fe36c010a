"""CPU restatement of the decode under a per-frame transition_bias (uis_frame_bias) for the tests.

The rule (include/uisrnn_hip.h): b[t] in [0, 1] is frame t's probability of a speaker change in the place of the model's
scalar; NaN means the model's own.  The step that decides frame t forms its priors from
(log(1 - b[t]), log(b[t]), log(b[t]) + log(crp_alpha)), float64 with the C library's log (math.log), log(0) = -inf.
Nothing else changes.

Built on tests/limit_ref.py: a (sub-)step is limit_ref's, given a VIEW of primed_ref.Model whose lp_stay and lp_sw are
that frame's (primed_ref.Hypothesis.candidate forms the new-cluster prior as lp_sw + l_alpha, the library's lp_new).

  view()       the model as frame t sees it
  step()       limit_ref.step with one view per frame of the window
  decode()     limit_ref.decode with a table: test_iteration (frame t % n, as mse0 is indexed), any look_ahead, limit
  Session      limit_ref.Session whose push takes the chunk's table
  score_one()  forced_ref.score_one with a table
  pattern()    the table the tests use
"""

import math

import numpy as np

import limit_ref
import nbest_ref
import primed_ref
from oracle import oracle

PATTERN = (float('nan'), 0.0, 0.5, 1.0, float('nan'), 0.0, 0.9)


def pattern(u, n):
  """b[u][t] = PATTERN[(t + u) % 7], and NaN at frame 0 where that would be 0 (no hypothesis has a previous label)."""
  b = np.array([PATTERN[(t + u) % len(PATTERN)] for t in range(n)], dtype=np.float64)
  if n and b[0] == 0.0:
    b[0] = np.nan
  return b


def log_pair(b):
  """(lp_stay, lp_sw) of a value in [0, 1]."""
  b = float(b)
  return (math.log(1.0 - b) if b < 1.0 else -math.inf), (math.log(b) if b > 0.0 else -math.inf)


class _View:
  """primed_ref.Model with one frame's lp_stay / lp_sw."""

  def __init__(self, model, b):
    self.__dict__.update(model.__dict__)
    self.lp_stay, self.lp_sw = log_pair(b)


def view(model, b):
  """The model for a frame whose table entry is b (None / NaN: the model itself)."""
  if b is None or math.isnan(float(b)):
    return model
  limit_ref._mse_params(model)   # pylint: disable=protected-access  (cached on the model before the view copies it)
  return _View(model, b)


def step(model, beam, xs, beam_size, limit=None, bs=None):
  """One window: xs [Lw, D] float32, bs the Lw table entries of its frames (None: no table).  limit_ref.step, with
  sub-step j's candidates and replay formed under view(model, bs[j])."""
  lw = xs.shape[0]
  if bs is None:
    return limit_ref.step(model, beam, xs, beam_size, limit)
  if lw == 1:
    return limit_ref.step(view(model, bs[0]), beam, xs, beam_size, limit)
  models = [view(model, b) for b in bs]
  mse_params = limit_ref._mse_params(model)   # pylint: disable=protected-access
  advance = limit_ref._advance                 # pylint: disable=protected-access
  cand, scores = [], []
  seen = [{} for _ in range(lw)]
  cache = {}

  def walk(b, hyp, j, path):
    for c in range(limit_ref.n_candidates(hyp, limit)):
      mean = hyp.means[c] if c < len(hyp.means) else model.m0
      if id(mean) not in seen[j]:
        seen[j][id(mean)] = oracle.weighted_mse(mse_params, mean, xs[j])
      sc = hyp.candidate(models[j], xs[j], c, seen[j])
      if j == lw - 1:
        cand.append((b, path + (c,)))
        scores.append(sc)
      else:
        walk(b, advance(models[j], hyp, xs[j], c, sc, cache, j), j + 1, path + (c,))

  for b, hyp in enumerate(beam):
    walk(b, hyp, 0, ())
  scores = np.array(scores, dtype=np.float32)
  finite = np.flatnonzero(np.isfinite(scores))
  order = finite[np.argsort(nbest_ref.score_key(scores[finite]), kind='stable')][:beam_size]
  out = []
  for i in order:
    b, path = cand[i]
    hyp = beam[b]
    for j, c in enumerate(path):
      hyp = advance(models[j], hyp, xs[j], c, hyp.candidate(models[j], xs[j], c, seen[j]), cache, j)
    assert hyp.score.view(np.uint32) == scores[i].view(np.uint32)
    out.append(hyp)
  return out


def decode(params, seq, beam_size, look_ahead=1, test_iteration=1, limit=None, bias=None, start=None):
  """limit_ref.decode with `bias`: None or float64 [N].  Returns its dict."""
  model = params if isinstance(params, primed_ref.Model) else primed_ref.Model(params)
  x = np.asarray(seq, dtype=np.float32)
  n = x.shape[0]
  total = int(test_iteration) * n
  beam = [start if start is not None else primed_ref.Hypothesis()]
  most = 0
  for t in range(0, total, int(look_ahead)):
    idx = [(t + j) % n for j in range(min(int(look_ahead), total - t))]
    xs = np.stack([x[i] for i in idx])
    beam = step(model, beam, xs, beam_size, limit, None if bias is None else [bias[i] for i in idx])
    most = max([most] + [len(h.means) for h in beam])
    if not beam:
      break
  if n == 0:
    labels, score = np.zeros(0, dtype=np.int32), np.float32(0.0)
  elif beam:
    labels, score = np.array(beam[0].trace[-n:], dtype=np.int32), beam[0].score
  else:
    labels, score = np.full(n, -1, dtype=np.int32), np.float32(np.inf)
  return {'labels': labels, 'score': np.float32(score),
          'beam_scores': primed_ref.padded_beam([h.score for h in beam] if n else [], beam_size),
          'max_clusters': most, 'beam': beam}


def decode_list(params, seqs, beam_size, look_ahead=1, test_iteration=1, limits=None, biases=None):
  """decode() of every sequence under its own limit and table, as oracle.decode returns a list's results."""
  model = primed_ref.Model(params)
  outs = [decode(model, s, beam_size, look_ahead, test_iteration, None if limits is None else limits[u],
                 None if biases is None else biases[u]) for u, s in enumerate(seqs)]
  return {'labels': [o['labels'] for o in outs], 'scores': np.array([o['score'] for o in outs], dtype=np.float32),
          'beam_scores': np.stack([o['beam_scores'] for o in outs]) if outs else np.zeros((0, beam_size), np.float32),
          'max_clusters': np.array([o['max_clusters'] for o in outs], dtype=np.int32), 'outs': outs}


class Session(limit_ref.Session):
  """One utterance of a session whose pushes may carry the chunk's table."""

  def push(self, chunk, bias=None):   # pylint: disable=arguments-differ
    x = np.asarray(chunk, dtype=np.float32)
    for t in range(x.shape[0]):
      if self.beam:
        self.beam = step(self.model, self.beam, x[t:t + 1], self.beam_size, self.limit,
                         None if bias is None else [bias[t]])
      self.received += 1


def score_one(params, seq, labels, bias=None):
  """forced_ref.score_one under a table: (score float32, per-frame losses float32 [N])."""
  x = np.asarray(seq, dtype=np.float32)
  n = x.shape[0]
  m0, h1 = oracle.constants(params)
  p0 = float(params['transition_bias'])
  alpha = float(params['crp_alpha'])
  l_alpha = math.log(alpha)
  means, hids, counts, blk = [], [], [], []
  last, sumblk = -1, 0
  losses = np.full(n, np.inf, dtype=np.float32)
  score = np.float32(0.0)
  for t in range(n):
    b = p0 if bias is None or math.isnan(float(bias[t])) else float(bias[t])
    lp_stay, lp_sw = (math.log(1.0 - p0), math.log(p0)) if b == p0 else log_pair(b)
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
    with np.errstate(invalid='ignore'):
      loss = np.float32(np.float64(mse) - prior)
    losses[t] = loss
    score = np.float32(score + loss)
    last = c
  return score, losses
