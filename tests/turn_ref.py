"""CPU restatement of the decode under a minimum turn length (uis_min_turn) for the tests.

The rule (include/uisrnn_hip.h): an utterance carries an integer m; 0 and 1 mean no rule.  A hypothesis' run is the number
of most recent decode steps of its trace -- the whole trace, tiled test_iteration times -- that carry its last label.  A
hypothesis that has a last label l and a run below m keeps candidate l only; one without a last label keeps every
candidate.  Nothing else changes.

Built on tests/known_ref.py: known_ref.step's walk, with one more filter in candidates().  The run is read off
hyp.trace, which holds every decode step so far (a window's sub-steps included: the prefix being extended).

  run()          the trailing run of a trace
  candidates()   known_ref.candidates under m
  decode()       any look_ahead, test_iteration, limit, bias and tags, plus m
  decode_list()  every sequence under its own tables
  turns()        the lengths of a trace's turns, in order
  rule_holds()   every completed turn of a trace has at least m steps
"""

import contextlib

import numpy as np

import known_ref
import primed_ref

_known_candidates = known_ref.candidates


def run(trace):
  """How many of the most recent entries of `trace` carry its last label (0 for an empty trace)."""
  n = 0
  while n < len(trace) and trace[-1 - n] == trace[-1]:
    n += 1
  return n


def candidates(hyp, limit, g, m):
  """known_ref.candidates(hyp, limit, g), of which only the last label survives while its run is below m."""
  allowed = _known_candidates(hyp, limit, g)
  if m and m >= 2 and hyp.trace and run(hyp.trace) < m:
    return [c for c in allowed if c == hyp.trace[-1]]
  return allowed


@contextlib.contextmanager
def _rule(m):
  """known_ref's walk with candidates() under m, for the time of one decode."""
  known_ref.candidates = lambda hyp, limit, g: candidates(hyp, limit, g, m)
  try:
    yield
  finally:
    known_ref.candidates = _known_candidates


def decode(params, seq, beam_size, look_ahead=1, test_iteration=1, limit=None, bias=None, tags=None, m=0):
  """known_ref.decode under the minimum turn length m.  Returns its dict."""
  with _rule(int(m)):
    return known_ref.decode(params, seq, beam_size, look_ahead, test_iteration, limit, bias, tags)


def decode_list(params, seqs, beam_size, look_ahead=1, test_iteration=1, limits=None, biases=None, tags=None, ms=None):
  """decode() of every sequence under its own limit, tables and m, as oracle.decode returns a list's results."""
  model = primed_ref.Model(params)
  outs = [decode(model, s, beam_size, look_ahead, test_iteration, None if limits is None else limits[u],
                 None if biases is None else biases[u], None if tags is None else tags[u], 0 if ms is None else ms[u])
          for u, s in enumerate(seqs)]
  return {'labels': [o['labels'] for o in outs], 'scores': np.array([o['score'] for o in outs], dtype=np.float32),
          'beam_scores': np.stack([o['beam_scores'] for o in outs]) if outs else np.zeros((0, beam_size), np.float32),
          'max_clusters': np.array([o['max_clusters'] for o in outs], dtype=np.int32), 'outs': outs}


def turns(trace):
  """The lengths of the turns of `trace`, in order."""
  out = []
  for t, c in enumerate(trace):
    if t and c == trace[t - 1]:
      out[-1] += 1
    else:
      out.append(1)
  return out


def rule_holds(trace, m):
  """Every completed turn of `trace` (all but the last) has at least m steps."""
  return all(n >= m for n in turns(trace)[:-1])
