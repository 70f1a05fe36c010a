"""CPU restatement of one slot of a session under a minimum turn length (uis_session_min_turn) for the tests.

tests/known_session_ref.py's Session -- the beam step under a tag, a bias entry and the slot's max_speakers, the commit
rule, retirement and the id map -- with the step's candidates filtered by tests/turn_ref.py's candidates() under the
slot's m.  m is the slot's: 0 and 1 mean no rule, and the slot is then known_session_ref.Session bit for bit.

The run of a hypothesis is min(turn_ref.run(trace), m) of its WHOLE trace: the reference keeps every frame of the stream,
committed ones included, and retire_ref renumbers the trace without changing which entries are equal, so the run survives
both by itself.  A hypothesis that arrived through an import or a prime may carry a run that its trace does not show (a
blob from a slot without a rule: run m; a run clamped by a smaller m): the override `turn_over` = (trace length when it
arrived, run it arrived with) says so, and the steps after it hand it on to the children.

  run_of()        the run of a hypothesis under m, override included
  candidates()    turn_ref.candidates, or the same filter on the overridden run
  last_word()     uis_blob_last_word: a blob's (label, run) as a slot with m holds it
  Session         push / commit / retire / retirable / bindings as known_session_ref; turns_row(); exported() / imported()
  primed()        the hypothesis uis_stream_prime leaves in a slot with m
"""

import numpy as np

import known_ref
import known_session_ref
import turn_ref

_known_candidates = known_ref.candidates   # (push() swaps the module's name for the time of its steps)


def run_of(hyp, m):
  """The run of `hyp` in a slot whose minimum turn length is m (0 where the slot has no rule or the trace is empty)."""
  if not m or m < 2 or not hyp.trace:
    return 0
  r = turn_ref.run(hyp.trace)
  over = getattr(hyp, 'turn_over', None)
  if over is not None:
    at, run_at = over
    tail = len(hyp.trace) - at
    if r > tail:        # every step since the arrival continues the label it arrived with
      r = tail + run_at
  return min(r, int(m))


def candidates(hyp, limit, g, m):
  """The clusters `hyp` may give a frame with tag g under m."""
  if getattr(hyp, 'turn_over', None) is None:
    return turn_ref.candidates(hyp, limit, g, m)
  allowed = _known_candidates(hyp, limit, g)
  if m and m >= 2 and hyp.trace and run_of(hyp, m) < m:
    return [c for c in allowed if c == hyp.trace[-1]]
  return allowed


def last_word(label, run, m):
  """uis_blob_last_word on (label, run): the (label, run) a slot with m holds after the import."""
  if label < 0:
    return -1, 0
  if m < 2:
    return int(label), 0
  return int(label), (int(m) if run == 0 or run > m else int(run))


def trailing_run(labels, m):
  """min(trailing run of `labels`, m): what uis_stream_prime writes into a slot with m >= 2; 0 without a rule."""
  return min(turn_ref.run([int(c) for c in labels]), int(m)) if m >= 2 and len(labels) else 0


def primed(model, frames, labels, tags=None):
  """known_session_ref.primed: the prefix is forced, whatever turns it holds; its trace shows the trailing run."""
  return known_session_ref.primed(model, frames, labels, tags)


class Session(known_session_ref.Session):
  """One slot of a session whose slot has the minimum turn length m."""

  def __init__(self, params, beam_size, start=None, limit=None, m=0):
    super().__init__(params, beam_size, start, limit)
    self.m = int(m)

  def push(self, chunk, tags=None, bias=None):
    if self.m < 2:
      return super().push(chunk, tags, bias)
    x = np.asarray(chunk, dtype=np.float32)
    keep = known_ref.candidates
    known_ref.candidates = lambda hyp, limit, g: candidates(hyp, limit, g, self.m)
    try:
      for t in range(x.shape[0]):
        if self.beam:
          parents = self.beam
          self.beam = known_ref.step(self.model, parents, x[t][None], self.beam_size, self.limit,
                                     None if bias is None else [bias[t]], None if tags is None else [tags[t]])
          for child in self.beam:   # (the members of one beam never carry the same trace: the parent is the one that matches)
            for parent in parents:
              if getattr(parent, 'turn_over', None) is not None and parent.trace == child.trace[:-1]:
                child.turn_over = parent.turn_over
        self.received += 1
    finally:
      known_ref.candidates = keep
    return None

  def retire(self, R):
    over = [getattr(h, 'turn_over', None) for h in self.beam]
    ids = super().retire(R)
    for h, o in zip(self.beam, over):   # (retire_hypothesis builds new objects; lengths and equalities of the trace stay)
      if o is not None:
        h.turn_over = o
    return ids

  def runs(self):
    """The run of every live hypothesis, best first."""
    return [run_of(h, self.m) for h in self.beam[:self.live]]

  def turns_row(self):
    """uis_session_turns' row of this slot: [last label of the best hypothesis (present numbering), its run]."""
    if not self.live or not self.beam or self.beam[0].last < 0:
      return [-1, 0]
    return [int(self.beam[0].last), run_of(self.beam[0], self.m)]

  def exported(self):
    """What a blob carries of the turn: (label, run) of every live rank's last-label word."""
    return [(int(h.last), run_of(h, self.m)) for h in self.beam[:self.live]]

  def imported(self, source, m=None):
    """This (fresh) slot after uis_stream_import of `source`'s blob: the source's state, each rank's word normalised
    against this slot's m.  Returns self."""
    assert self.received == 0
    m = self.m if m is None else int(m)
    words = source.exported()
    self.beam = []
    for h, (label, run) in zip(source.beam[:source.live], words):
      c = h.copy()
      if hasattr(h, 'tags'):
        c.tags = h.tags
      _, arrived = last_word(label, run, m)
      if m >= 2 and label >= 0:
        c.turn_over = (len(c.trace), arrived)
      self.beam.append(c)
    self.received, self.committed = source.received, source.committed
    self.final, self.gone = list(source.final), list(source.gone)
    self.m = m
    return self
