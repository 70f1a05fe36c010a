"""CPU restatement of one slot of a session pushed under speaker tags (uis_stream_speakers) for the tests.

tests/retire_ref.py's Session -- commit_ref's beam search from a beam, the commit rule, retirement and the id map --
with the beam step replaced by tests/known_ref.py's step under one frame's tag, bias entry and the slot's max_speakers:

  push(chunk, tags, bias)   known_ref.step(model, beam, x[None], beam_size, limit, [b], [g]) per frame
  retire_hypothesis()       retire_ref's list surgery, and the hypothesis' `tags` tuple loses the same entries: a
                            binding follows its cluster's new index
  retirable()               retire_ref's rule minus the clusters that carry a tag in any live hypothesis
  bindings()                {tag: present cluster index} of the best hypothesis, from known_ref.tags_of(beam[0])
  primed()                  the hypothesis uis_stream_prime leaves under tags: primed_ref.advance_forced along the labels,
                            bound as the decode would bind it; ValueError where the labels contradict the tags

Without tags, and with all-zero tags, this is retire_ref.Session bit for bit (tests/test_known_session_host.py).
"""

import numpy as np

import known_ref
import primed_ref
import retire_ref


def retire_hypothesis(hyp, R, committed):
  """retire_ref.retire_hypothesis, and the binding without the entries in R."""
  tags = known_ref.tags_of(hyp)
  drop = {int(k) for k in R}
  assert not any(tags[k] for k in drop), 'a tagged cluster is not retirable'
  out = retire_ref.retire_hypothesis(hyp, R, committed)
  out.tags = tuple(g for k, g in enumerate(tags) if k not in drop)
  return out


def bind_prefix(labels, tags):
  """The binding after `labels` (first-appearance form) under `tags`: one tag per cluster, 0 = none.  ValueError where
  the relation tag <-> label is no partial bijection (the decode's rule admits no such trace)."""
  of_label, of_tag = {}, {}
  for t, (c, g) in enumerate(zip(labels, tags)):
    c, g = int(c), int(g)
    if not g:
      continue
    if of_label.get(c, g) != g or of_tag.get(g, c) != c:
      raise ValueError('the prefix labels contradict its tags (frame {})'.format(t))
    of_label[c], of_tag[g] = g, c
  k = max([int(c) for c in labels], default=-1) + 1
  return tuple(of_label.get(c, 0) for c in range(k))


def primed(model, frames, labels, tags=None):
  """The start hypothesis of a slot primed with `labels` over `frames` under `tags` (None: no table)."""
  hyp = primed_ref.advance_forced(model, frames, labels)
  if tags is not None:
    hyp.tags = bind_prefix(labels, tags)
  return hyp


class Session(retire_ref.Session):
  """One slot of a session whose pushes may carry tags, a bias table and a speaker bound."""

  def __init__(self, params, beam_size, start=None, limit=None):
    super().__init__(params, beam_size, start)
    self.limit = limit

  def push(self, chunk, tags=None, bias=None):
    x = np.asarray(chunk, dtype=np.float32)
    for t in range(x.shape[0]):
      if self.beam:
        self.beam = known_ref.step(self.model, self.beam, x[t][None], self.beam_size, self.limit,
                                   None if bias is None else [bias[t]], None if tags is None else [tags[t]])
      self.received += 1

  def tagged(self):
    """Present indices that carry a tag in any live hypothesis."""
    return sorted({k for h in self.beam[:self.live] for k, g in enumerate(known_ref.tags_of(h)) if g})

  def retirable(self):
    held = set(self.tagged())
    return [k for k in super().retirable() if k not in held]

  def retire(self, R):
    R = sorted(int(k) for k in R)
    assert len(set(R)) == len(R) and set(R) <= set(self.retirable()), (R, self.retirable())
    ids = [retire_ref.to_global(k, self.gone) for k in R]
    if R:
      self.beam = [retire_hypothesis(h, R, self.committed) for h in self.beam]
      self.gone = sorted(self.gone + ids)
    self.retired.append(ids)
    return ids

  def bindings(self):
    """{tag: present cluster index} of the best hypothesis ({}: no live hypothesis)."""
    if not self.beam:
      return {}
    return {int(g): k for k, g in enumerate(known_ref.tags_of(self.beam[0])) if g}

  def bindings_row(self):
    """uis_stream_bindings' row of this slot: int32 [128]."""
    row = np.full(128, -1, dtype=np.int32)
    bound = self.bindings()
    row[0] = len(bound)
    for g, k in bound.items():
      row[g] = k
    return row
