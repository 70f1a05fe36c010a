"""CPU restatement of the decode under a per-utterance speaker bound (max_speakers) for the tests.

The rule (include/uisrnn_hip.h): a hypothesis that already holds K >= limit clusters has no new-cluster candidate --
what the reference's beam search would do if _calculate_score gave +inf to the new-cluster entry of such a state.
Nothing else changes.  limit None or 0: no bound.

Built on tests/primed_ref.py's Model / Hypothesis (bit-exact against the oracle, made only of oracle.rnn_step,
oracle.weighted_mse and oracle.constants):

  decode()   predict_single (uisrnn/uisrnn.py:479-562) with `limit`, test_iteration and any look_ahead.  A window of
             Lw frames scores every tuple (c_1 .. c_Lw) of every beam hypothesis, c_j among the clusters of the prefix
             that (c_1 .. c_{j-1}) built plus -- where that prefix holds fewer than `limit` -- a new one
             (_calculate_score, uisrnn.py:455-477: the tuples in row-major order, hypothesis by hypothesis); the finite
             ones are sorted stably by nbest_ref.score_key and the leading min(#finite, beam_size) are replayed
             (uisrnn.py:551-559).  With no limit this is oracle.decode bit for bit (tests/test_limit_host.py).
  Session    retire_ref.Session whose limit may change between pushes.

A cluster state met twice in a step (hypotheses share them, like the reference's shallow list copies) is advanced
once: the result depends on the state and the frame alone.
"""

import numpy as np

import nbest_ref
import primed_ref
import retire_ref
from oracle import oracle


def _mse_params(model):
  """The model with a GRU of one hidden unit: oracle.weighted_mse reads observation_dim and sigma2 only, and the
  oracle's wrappers rebuild their model from the parameters at every call."""
  if not hasattr(model, 'mse_params'):
    p = model.params
    dim = int(p['observation_dim'])
    zeros = lambda *shape: np.zeros(shape, dtype=np.float32)   # pylint: disable=unnecessary-lambda-assignment
    model.mse_params = {
        'observation_dim': dim, 'rnn_hidden_size': 1, 'rnn_depth': 1, 'sigma2': p['sigma2'],
        'transition_bias': p['transition_bias'], 'crp_alpha': p['crp_alpha'],
        'gru_weight_ih': [zeros(3, dim)], 'gru_weight_hh': [zeros(3, 1)], 'gru_bias_ih': [zeros(3)],
        'gru_bias_hh': [zeros(3)], 'linear_mean1_weight': zeros(1, 1), 'linear_mean1_bias': zeros(1),
        'linear_mean2_weight': zeros(dim, 1), 'linear_mean2_bias': zeros(dim), 'rnn_init_hidden': zeros(1, 1)}
  return model.mse_params


def _unbounded(limit):
  return limit is None or int(limit) <= 0


def n_candidates(hyp, limit):
  """Clusters hypothesis `hyp` may give the next frame to: 0 .. K - 1, and K while K is below the limit."""
  k = len(hyp.means)
  return k + 1 if _unbounded(limit) or k < int(limit) else k


def _advance(model, hyp, x, c, score, cache, key):
  """hyp.advance(model, x, c, score) with the cluster state's update shared between the hypotheses that share the
  state (cache: per frame; key: which frame of the window)."""
  if cache is None:
    return hyp.advance(model, x, c, score)
  src = hyp.hids[c] if c < len(hyp.means) else None
  slot = (key, id(src) if src is not None else -1)
  if slot not in cache:
    out = hyp.advance(model, x, c, score)
    cache[slot] = (src, out.means[c], out.hids[c], out.counts[c])   # (src kept alive: its id names the entry)
    return out
  _, mean, hid, count = cache[slot]
  h = hyp.copy()
  h.score = np.float32(score)
  if c < len(hyp.means):
    h.means[c], h.hids[c], h.counts[c] = mean, hid, count
    if c != hyp.last:
      h.blk[c] += 1
      h.sumblk += 1
  else:
    h.means.append(mean)
    h.hids.append(hid)
    h.counts.append(count)
    h.blk.append(1)
    h.sumblk += 1
  h.last = c
  h.trace.append(c)
  return h


def step(model, beam, xs, beam_size, limit=None):
  """One window: xs [Lw, D] float32.  Returns the next beam, best first."""
  lw = xs.shape[0]
  cand, scores = [], []
  seen = [{} for _ in range(lw)]
  cache = {}

  mse_params = _mse_params(model)

  def walk(b, hyp, j, path):
    for c in range(n_candidates(hyp, limit)):
      mean = hyp.means[c] if c < len(hyp.means) else model.m0
      if id(mean) not in seen[j]:   # (Hypothesis.candidate finds it there)
        seen[j][id(mean)] = oracle.weighted_mse(mse_params, mean, xs[j])
      sc = hyp.candidate(model, xs[j], c, seen[j])
      if j == lw - 1:
        cand.append((b, path + (c,)))
        scores.append(sc)
      else:
        walk(b, _advance(model, hyp, xs[j], c, sc, cache, j), j + 1, path + (c,))

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
      hyp = _advance(model, hyp, xs[j], c, hyp.candidate(model, xs[j], c, seen[j]), cache, j)
    assert hyp.score.view(np.uint32) == scores[i].view(np.uint32)
    out.append(hyp)
  return out


def decode(params, seq, beam_size, look_ahead=1, test_iteration=1, limit=None, start=None):
  """Returns dict(labels int32 [N], score, beam_scores float32 [beam_size] (+inf padded), max_clusters, beam: the
  final hypotheses)."""
  model = params if isinstance(params, primed_ref.Model) else primed_ref.Model(params)
  x = np.asarray(seq, dtype=np.float32)
  n = x.shape[0]
  total = int(test_iteration) * n
  beam = [start if start is not None else primed_ref.Hypothesis()]
  most = 0
  for t in range(0, total, int(look_ahead)):
    xs = np.stack([x[(t + j) % n] for j in range(min(int(look_ahead), total - t))])
    beam = step(model, beam, xs, beam_size, limit)
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


def decode_list(params, seqs, beam_size, look_ahead=1, test_iteration=1, limits=None):
  """decode() of every sequence under its own limit, as oracle.decode returns a list's results."""
  model = primed_ref.Model(params)
  outs = [decode(model, s, beam_size, look_ahead, test_iteration, None if limits is None else limits[u])
          for u, s in enumerate(seqs)]
  return {'labels': [o['labels'] for o in outs], 'scores': np.array([o['score'] for o in outs], dtype=np.float32),
          'beam_scores': np.stack([o['beam_scores'] for o in outs]) if outs else np.zeros((0, beam_size), np.float32),
          'max_clusters': np.array([o['max_clusters'] for o in outs], dtype=np.int32), 'outs': outs}


def primed_decode(params, seq, prefix_labels, beam_size, limit=None):
  """primed_ref.primed_decode under a limit: the prefix is forced whatever its cluster count."""
  model = primed_ref.Model(params)
  p = len(prefix_labels)
  start = primed_ref.advance_forced(model, seq[:p], prefix_labels)
  if seq.shape[0] > p:
    beam = decode(model, seq[p:], beam_size, limit=limit, start=start)['beam']
  else:
    beam = [start]
  return {'labels': np.array([h.trace for h in beam], dtype=np.int32).reshape(len(beam), seq.shape[0]),
          'scores': np.array([h.score for h in beam], dtype=np.float32)}


class Session(retire_ref.Session):
  """One utterance of a session whose limit can change between pushes, and which can commit and retire."""

  def __init__(self, params, beam_size, limit=None, start=None):
    super().__init__(params, beam_size, start)
    self.limit = limit

  def set_limit(self, limit):
    self.limit = limit

  def push(self, chunk):
    x = np.asarray(chunk, dtype=np.float32)
    for t in range(x.shape[0]):
      if self.beam:
        self.beam = step(self.model, self.beam, x[t:t + 1], self.beam_size, self.limit)
      self.received += 1
