"""CPU restatement of the decode under partial speaker labels (uis_frame_speakers) for the tests.

The rule (include/uisrnn_hip.h): every frame carries a tag, 0 for unknown, 1 .. 127 for a known speaker, and every
hypothesis a partial, injective binding of tags to its clusters.  At a frame with tag g > 0 a hypothesis with K clusters
has these candidates: if g is bound to cluster c*, only c*; otherwise the clusters c < K that carry no tag, and the new
cluster K where max_speakers allows one -- the candidate that is taken binds g to its cluster.  At a frame with tag 0
every candidate is the untagged decode's, and nothing is bound.  Nothing else changes.

Built on tests/limit_ref.py and tests/bias_ref.py: a window is limit_ref.step's walk, with bias_ref's view of the model
per frame, and the binding is a tuple beside each hypothesis' clusters (`tags`, one entry per cluster, 0 = none; a
hypothesis without the attribute has bound nothing).

  candidates()  the clusters a hypothesis may give a frame with tag g
  step()        one window under tags, a per-frame bias and a limit
  decode()      any look_ahead, test_iteration (frame t % n, as mse0 is indexed; bindings persist), limit, bias
  decode_list() every sequence under its own tables
  pattern()     the table the GPU tests use
  first_appearance()  a tag sequence as the labels it forces
"""

import numpy as np

import bias_ref
import limit_ref
import nbest_ref
import primed_ref
from oracle import oracle


def pattern(u, n):
  """tags[u][t] = ((t + u) // 5) % 3 + 1 where (t + u) % 3 == 0, else 0."""
  return np.array([((t + u) // 5) % 3 + 1 if (t + u) % 3 == 0 else 0 for t in range(n)], dtype=np.uint8)


def first_appearance(tags):
  """The labels a fully tagged sequence forces: its tags numbered in the order they first appear."""
  seen = {}
  return np.array([seen.setdefault(int(g), len(seen)) for g in tags], dtype=np.int32)


def tags_of(hyp):
  """The binding of `hyp`: one tag per cluster, 0 = the cluster carries none."""
  tags = tuple(getattr(hyp, 'tags', ()))
  return tags + (0,) * (len(hyp.means) - len(tags))


def candidates(hyp, limit, g):
  """The clusters `hyp` may give a frame with tag g (0: unknown), in ascending order."""
  k = len(hyp.means)
  free = list(range(limit_ref.n_candidates(hyp, limit)))
  if not g:
    return free
  tags = tags_of(hyp)
  if g in tags:
    return [tags.index(g)]
  return [c for c in free if c >= k or tags[c] == 0]


def _bound(parent, child, c, g):
  """`child` = `parent` after a frame with tag g went to cluster c: the binding follows."""
  tags = list(tags_of(parent))
  if c == len(tags):
    tags.append(0)
  if g:
    tags[c] = int(g)
  child.tags = tuple(tags)
  return child


def step(model, beam, xs, beam_size, limit=None, bs=None, gs=None):
  """One window: xs [Lw, D] float32, bs the Lw bias entries of its frames (None: no table), gs its Lw tags (None: no
  table).  Returns the next beam, best first."""
  lw = xs.shape[0]
  gs = [0] * lw if gs is None else [int(g) for g in gs]
  models = [model if bs is None else bias_ref.view(model, b) for b in ([None] * lw if bs is None else bs)]
  mse_params = limit_ref._mse_params(model)   # pylint: disable=protected-access
  advance = limit_ref._advance                 # pylint: disable=protected-access
  cand, scores = [], []
  seen = [{} for _ in range(lw)]
  cache = {}

  def walk(b, hyp, j, path):
    for c in candidates(hyp, limit, gs[j]):
      mean = hyp.means[c] if c < len(hyp.means) else model.m0
      if id(mean) not in seen[j]:
        seen[j][id(mean)] = oracle.weighted_mse(mse_params, mean, xs[j])
      sc = hyp.candidate(models[j], xs[j], c, seen[j])
      if j == lw - 1:
        cand.append((b, path + (c,)))
        scores.append(sc)
      else:
        walk(b, _bound(hyp, advance(models[j], hyp, xs[j], c, sc, cache, j), c, gs[j]), j + 1, path + (c,))

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
      nxt = advance(models[j], hyp, xs[j], c, hyp.candidate(models[j], xs[j], c, seen[j]), cache, j)
      hyp = _bound(hyp, nxt, c, gs[j])
    assert hyp.score.view(np.uint32) == scores[i].view(np.uint32)
    out.append(hyp)
  return out


def decode(params, seq, beam_size, look_ahead=1, test_iteration=1, limit=None, bias=None, tags=None, start=None):
  """limit_ref.decode with `bias` (None or float64 [N]) and `tags` (None or ints [N]).  Returns its dict."""
  model = params if isinstance(params, primed_ref.Model) else primed_ref.Model(params)
  x = np.asarray(seq, dtype=np.float32)
  n = x.shape[0]
  total = int(test_iteration) * n
  beam = [start if start is not None else primed_ref.Hypothesis()]
  most = 0
  for t in range(0, total, int(look_ahead)):
    idx = [(t + j) % n for j in range(min(int(look_ahead), total - t))]
    xs = np.stack([x[i] for i in idx])
    beam = step(model, beam, xs, beam_size, limit, None if bias is None else [bias[i] for i in idx],
                None if tags is None else [tags[i] for i in idx])
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


def decode_list(params, seqs, beam_size, look_ahead=1, test_iteration=1, limits=None, biases=None, tags=None):
  """decode() of every sequence under its own limit and tables, as oracle.decode returns a list's results."""
  model = primed_ref.Model(params)
  outs = [decode(model, s, beam_size, look_ahead, test_iteration, None if limits is None else limits[u],
                 None if biases is None else biases[u], None if tags is None else tags[u]) for u, s in enumerate(seqs)]
  return {'labels': [o['labels'] for o in outs], 'scores': np.array([o['score'] for o in outs], dtype=np.float32),
          'beam_scores': np.stack([o['beam_scores'] for o in outs]) if outs else np.zeros((0, beam_size), np.float32),
          'max_clusters': np.array([o['max_clusters'] for o in outs], dtype=np.int32), 'outs': outs}
