"""tests/policy_walk.py's small plan on a session whose slots carry minimum turn lengths: its trace on the CPU reference.
No device, no library.

The PLAN is policy_walk's, imported and not edited: PLANS['small'] with CASES['small4']'s arguments -- pushes with every
kind of bias table (a non-finite frame, a table left pending by a refusal), commits with and without horizons,
restarts, primes, uis_stream_limits, retirements (query, all, subset), moves between slots and every refusal.  Here it
runs on tests/turn_session_ref.py's Session, one per slot, and three things differ from policy_walk.trace:

  the values   slot u opens under VALUES[u % 4]; after every restart of the plan (and for the source slot of a move) the
               slot, fresh again, gets its next value of VALUES (a 'setm' step of its own behind the operation), so a
               slot decodes its successive utterances under different values and a move crosses from one value to
               another: the import normalises the runs against the target slot's
  the cap      the session opens with max_clusters 16 and the sequences are tests/turn_session_cases.py's kind, whose
               decodes stay far below it (asserted), so nothing has to steer; the plan's own `cap` argument (6) still
               sets its limits and the length of its prefixes
  the readout  snapshots are turn_session_cases.snap's -- the window's n-best rows in the present numbering, the scores'
               bits, uis_session_turns' row, every live rank's (label, run), the frame counts -- plus the slot's limit

trace() returns the steps: dict(op, kind, call, result, snap); facts() what the walk is meant to reach.
"""

import functools
import types

import numpy as np

import golden_util
import policy_walk as pw
import primed_ref
import session_walk as sw
import turn_session_cases as tc
import turn_session_ref as tsr
from oracle import oracle
from uisrnn_amd import synth

CASE = 'small4'
VALUES = (0, 2, 3, 5)
MAX_CLUSTERS = 16
LIVES = 8
SEQ_LEN = 200
INVALID_ARG, UNSUPPORTED = pw.INVALID_ARG, pw.UNSUPPORTED


@functools.lru_cache(maxsize=None)
def shape():
  case = pw.CASES[CASE]
  oracle.lib()
  params = golden_util.load_case(case['model'])['params']
  dim = int(params['observation_dim'])
  pool = [[synth.make_utterance(9500 + 100 * u + k, SEQ_LEN, dim, mean_segment=2.0) for k in range(LIVES)]
          for u in range(case['n_utt'])]
  plan = pw.PLANS[case['plan']](case['n_utt'], case['window'], case['cap'], case['seed'])
  return types.SimpleNamespace(name=CASE, params=params, model=primed_ref.Model(params), n_utt=case['n_utt'], beam=case['beam'],
                               window=case['window'], cap=MAX_CLUSTERS, plan_cap=case['cap'], pool=pool, plan=plan)


class _Slot:
  """One utterance: its reference session, its sequence and how much of it is used up."""

  def __init__(self, sh, u, life, limit, m):
    self.seq, self.truth = sh.pool[u][life % LIVES]
    self.pos = 0
    self.ref = tsr.Session(sh.model, sh.beam, None, limit or None, m)

  @property
  def dead(self):
    return self.ref.received > 0 and not self.ref.beam


def snap(slots, limits):
  out = tc.snap([s.ref for s in slots])
  for col, lim in zip(out, limits):
    col['limit'] = int(lim)
  return out


@functools.lru_cache(maxsize=None)
def trace():
  sh = shape()
  n_utt, window = sh.n_utt, sh.window
  p0 = float(sh.params['transition_bias'])
  limits = [0] * n_utt
  values = [VALUES[u % 4] for u in range(n_utt)]
  lives = [0] * n_utt
  turn = [u for u in range(n_utt)]   # which of VALUES a slot takes next

  def begin(u):
    slot = _Slot(sh, u, lives[u], limits[u], values[u])
    lives[u] += 1
    return slot

  slots = [begin(u) for u in range(n_utt)]
  steps = []

  def record(op, kind, call, result):
    steps.append({'op': op, 'kind': kind, 'call': call, 'result': result, 'snap': snap(slots, limits)})
    assert all(col['K'] < MAX_CLUSTERS for col in steps[-1]['snap']), (len(steps), op, 'the cluster cap is in reach')

  def setm(fresh):
    """The slots in `fresh` have received nothing: each takes its next value."""
    for u in fresh:
      assert slots[u].ref.received == 0
      turn[u] += 1
      values[u] = VALUES[turn[u] % 4]
      slots[u].ref.m = values[u]
    record(('setm', tuple(values)), 'setm', {'values': list(values)}, None)

  def sizes(wants):
    out = []
    for u, s in enumerate(slots):
      room, left = window - s.ref.have, len(s.seq) - s.pos
      out.append(min(room, left) if wants[u] == 'fill' else min(int(wants[u]), room, left))
    return out

  def peek(wants):
    return [np.array(s.seq[s.pos:s.pos + n], dtype=np.float64) if n else None for s, n in zip(slots, sizes(wants))]

  def whole_table(chunks, tables):
    if all(pw.kind_of(tables[u]) == 'none' for u in range(n_utt) if chunks[u] is not None):
      return None, [None] * n_utt
    per = [None if c is None else pw._table(tables[u], len(c), p0) for u, c in enumerate(chunks)]   # pylint: disable=protected-access
    return np.concatenate([t for t in per if t is not None]), per

  record(('setm', tuple(values)), 'setm', {'values': list(values)}, None)
  for op in sh.plan:
    kind = op[0]
    if kind == 'push':
      wants, tables = op[1], op[2]
      bad = op[3] if len(op) > 3 else None
      pending = bool(op[4]) if len(op) > 4 else False
      chunks = peek(wants)
      assert bad is None or chunks[bad] is not None, 'the non-finite frame was clipped away'
      if bad is not None:
        chunks[bad][0, 0] = np.inf
      bias, per = whole_table(chunks, tables)
      for u, (s, part) in enumerate(zip(slots, chunks)):
        if part is None:
          continue
        s.pos += len(part)
        tab = per[u] if pw.kind_of(tables[u]) != 'none' else None
        with np.errstate(all='ignore'):
          s.ref.push(part, None, tab)
      record(op, 'push', {'chunks': chunks, 'bias': None if pending else bias, 'pending': pending}, None)
    elif kind == 'commit':
      horizons = None if op[1] is None else [int(v) for v in op[1]]
      out = [s.ref.commit(None if horizons is None or horizons[u] < 0 else horizons[u]) for u, s in enumerate(slots)]
      record(op, 'commit', {'horizons': horizons},
             {'labels': [[tsr.known_session_ref.retire_ref.to_local(c, s.ref.gone) for c in o[0]] for o, s in zip(out, slots)],
              'dropped': [o[1] for o in out]})
    elif kind == 'restart':
      for u in op[1]:
        slots[u] = begin(u)
      record(op, 'restart', {'which': [u in op[1] for u in range(n_utt)]}, None)
      setm(sorted(op[1]))
    elif kind == 'prime':
      chunks, labels, result = [None] * n_utt, [None] * n_utt, {}
      for u, (source, n) in sorted(op[1].items()):
        s = slots[u]
        assert s.ref.received == 0 and s.pos == 0
        frames = np.array(s.seq[:int(n)], dtype=np.float64)
        s.pos = int(n)
        if source == 'truth':
          lab = sw.first_appearance(s.truth[:int(n)])
        else:
          lab = [int(v) for v in oracle.decode(sh.model.params, [frames], 1, 1, 1)['labels'][0]]
        lab = np.array(lab, dtype=np.int32)
        start = tsr.primed(sh.model, frames, lab)
        s.ref = tsr.Session(sh.model, sh.beam, start, limits[u] or None, values[u])
        chunks[u], labels[u], result[u] = frames, lab, int(tc._bits(start.score)[0])   # pylint: disable=protected-access
      record(op, 'prime', {'chunks': chunks, 'labels': labels}, result)
    elif kind == 'limits':
      for u, v in enumerate(op[1]):
        limits[u] = int(v)
        slots[u].ref.limit = int(v) or None
      record(op, 'limits', {'limits': list(limits)}, None)
    elif kind == 'retire':
      able = [s.ref.retirable() for s in slots]
      if op[1] == 'query':
        picks = [[] for _ in range(n_utt)]
      elif op[1] == 'all':
        picks = able
      else:
        rng = np.random.default_rng(op[2])
        picks = [[k for k in a if rng.random() < 0.5] for a in able]
      for s, pick in zip(slots, picks):
        s.ref.retire(pick)
      record(op, 'retire', {'clusters': None if op[1] == 'all' else [list(p) or None for p in picks]},
             {'retired': [list(p) for p in picks], 'K': [s.ref.K() for s in slots], 'retirable': able})
    elif kind == 'move':
      src, dst = int(op[1]), int(op[2])
      if slots[src].dead:
        record(op, 'move_refused', {'src': src, 'dst': dst}, INVALID_ARG)
        continue
      moved = slots[src]
      crossing = (values[src], values[dst], [list(w) for w in moved.ref.exported()])
      moved.ref = tsr.Session(sh.model, sh.beam, None, limits[dst] or None, values[dst]).imported(moved.ref)
      slots[dst] = moved
      slots[src] = begin(src)
      record(op, 'move', {'src': src, 'dst': dst}, {'from_m': crossing[0], 'to_m': crossing[1], 'words': crossing[2]})
      setm([src])
    elif kind == 'refuse':
      what = op[1]
      dim = slots[0].seq.shape[1]
      if what in ('push', 'bias_push_long'):
        u = op[2]
        n = window - slots[u].ref.have + int(op[3])
        chunks = [np.array(slots[v].seq[slots[v].pos:slots[v].pos + 1], dtype=np.float64) if window > slots[v].ref.have else None
                  for v in range(n_utt)]
        chunks[u] = np.zeros((n, dim))
        bias = np.full(sum(len(c) for c in chunks if c is not None), 0.5) if what == 'bias_push_long' else None
        call, result = {'call': 'push', 'chunks': chunks, 'bias': bias}, INVALID_ARG
      elif what in ('prime_received', 'prime_long', 'bias_prime'):
        u = op[2]
        n = window + 1 if what == 'prime_long' else 2
        assert (slots[u].ref.received == 0) == (what != 'prime_received'), (what, u)
        chunks, labels = [None] * n_utt, [None] * n_utt
        chunks[u], labels[u] = np.tile(np.array(slots[u].seq[:1], dtype=np.float64), (n, 1)), np.zeros(n, dtype=np.int32)
        call = {'call': 'prime', 'chunks': chunks, 'labels': labels, 'bias': np.full(n, 0.5) if what == 'bias_prime' else None}
        result = UNSUPPORTED if what == 'bias_prime' else INVALID_ARG
      elif what == 'bias_length':
        chunks = peek(op[2])
        total = sum(len(c) for c in chunks if c is not None)
        assert total >= 2, op
        call, result = {'call': 'push', 'chunks': chunks, 'bias': np.full(total - 1, 0.25)}, INVALID_ARG
      elif what == 'limits_range':
        call, result = {'call': 'limits', 'limits': [int(v) for v in op[2]]}, INVALID_ARG
      elif what == 'bias_value':
        stays, _ = whole_table(peek(op[2]), op[3])
        call, result = {'call': 'frame_bias', 'stays': stays, 'bias': np.array([0.5, 1.5])}, INVALID_ARG
      else:
        raise ValueError(op)
      record(op, 'refuse', call, result)
      assert steps[-1]['snap'] == steps[-2]['snap']
    else:
      raise ValueError(op)
  return steps


def facts(steps):
  """What the walk reaches, for tests/test_turn_session_host.py to assert."""
  out = {'kinds': sorted({st['kind'] for st in steps}), 'held_after_commit': 0, 'held_after_retire': 0, 'retired_under_rule': 0,
         'crossings': set(), 'clamped_or_loosened': 0, 'values_seen': [set() for _ in steps[0]['snap']], 'dead': 0,
         'held_pushes': 0, 'primed_under_rule': 0, 'limits_changed_mid_stream': 0}
  for i, st in enumerate(steps):
    for u, col in enumerate(st['snap']):
      out['values_seen'][u].add(col['m'])
      held = col['m'] >= 2 and col['live'] and col['turns'][1] < col['m']
      if held and st['kind'] == 'commit':
        out['held_after_commit'] += 1
      if held and st['kind'] == 'retire' and st['result']['retired'][u]:
        out['held_after_retire'] += 1
      if held and st['kind'] == 'push' and st['call']['chunks'][u] is not None:
        out['held_pushes'] += 1
      if st['kind'] == 'retire' and st['result']['retired'][u] and col['m'] >= 2:
        out['retired_under_rule'] += 1
      if st['kind'] == 'prime' and st['call']['labels'][u] is not None and col['m'] >= 2:
        out['primed_under_rule'] += 1
      if st['kind'] == 'limits' and i and col['limit'] != steps[i - 1]['snap'][u]['limit'] and col['have'] + col['committed'] and col['m'] >= 2:
        out['limits_changed_mid_stream'] += 1
      out['dead'] += int(st['kind'] == 'push' and col['have'] > 0 and not col['live'])
    if st['kind'] == 'move':
      res = st['result']
      out['crossings'].add((res['from_m'], res['to_m']))
      after = st['snap'][st['call']['dst']]['words']
      out['clamped_or_loosened'] += int(after != res['words'])
  return out
