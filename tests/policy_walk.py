"""Model-based walks over a streaming session under speaker bounds and per-frame turn priors: plans, and their trace
on the CPU reference.  No device, no library.  The fourth walk, in tests/session_walk.py's form.

A PLAN is a deterministic list of operations on an n_utt-slot session: a scripted prologue that forces the rare
states, then a body drawn from np.random.default_rng(seed).  session_walk's operations stay as they are there (commit,
restart, prime, its three refusals); these are new or wider:

  ('push', wants, tables[, bad[, pending]])   tables[u]: the table of slot u's new frames -- 'none' (no entry: NaN rows
                             where other slots have entries), 'nan' (all NaN), 'p0' (exactly the model's
                             transition_bias), ('soft', values) (uniform in (0, 1), drawn by the plan's RNG: the leading
                             entries are used), ('hard', k) (bias_ref.pattern(k, n): 0, 1, 0.5, 0.9 and NaN) or
                             ('raw', values) (scripted values, NaN behind them).  Silent slots contribute no rows.
                             pending: the table was left pending by the 'bias_value' refusal before, the push itself
                             passes none.
  ('limits', values)         uis_stream_limits: one int per slot, from {0, 1, 2, 3, cap}
  ('retire', mode[, seed])   'query', 'all', or 'subset' (each retirable cluster with probability 1/2, decided while
                             tracing from the reference's retirable set, by default_rng(seed))
  ('move', src, dst)         export src, restart dst, import into dst, restart src: the utterance goes on under dst's
                             limit.  Where src's beam is empty the export is refused and nothing else happens.
  ('refuse', what, ...)      'bias_length' (wants): a table one row short; 'bias_push_long' (slot, extra): a table of the
                             right length on a push beyond the window; 'bias_prime' (slot): a pending table before a valid
                             prime; 'limits_range' (values): one value 4097; 'bias_value' (wants, tables): a table
                             holding 1.5 behind a valid pending one, which stays (the push that follows runs under it
                             without passing one); 'bias_push_persistent' (wants): a table in a persistent session.
                             Every refusal is followed by a push without a table argument to the slots it named
                             (where their window has room): it must run on the model's value, bit for bit.

trace() runs a plan on tests/bias_ref.py's Session (which is limit_ref's and retire_ref's), one per slot.  Labels are in
the numbering the device hands them out in: a commit's labels in the numbering of its moment, the window's in the
present one (what test_gpu_restart._Session.snapshot keeps).  The trace steers: an unbounded slot that could pass the
cluster cap with the frames of the next push (at least three) commits and retires first and, where that does not
help, restarts -- as extra steps ('steer', ...) of the trace; its push is clipped to the clusters it has left.  The window needs no steering: a push is clipped to the room
it has, as in session_walk.  A slot whose limit is at most the cap is never steered: it reaches K == cap and stays.
facts() says which of the states the walk is meant for a trace reaches; tests/test_policy_walk_host.py asserts them.
"""

import functools

import numpy as np

import bias_ref
import golden_util
import primed_ref
import retire_ref
import session_walk as sw
from oracle import oracle

INVALID_ARG, UNSUPPORTED = -1, -7   # UIS_ERR_INVALID_ARG, UIS_ERR_UNSUPPORTED of include/uisrnn_hip.h
KEYS = sw.PER_UTT + ('received', 'committed', 'limit')
TABLE_KINDS = ('none', 'nan', 'soft', 'hard', 'p0')
OP_KINDS = ('push', 'commit_none', 'commit_h', 'restart', 'prime', 'refuse', 'limits', 'retire', 'move')
REFUSALS = ('push', 'prime_received', 'prime_long', 'bias_length', 'bias_push_long', 'bias_prime', 'limits_range', 'bias_value')
NAN = float('nan')

# name: the model (a tests/golden case), slots x beam x window, the plan and its seed, max_clusters, the pools
CASES = {
    'small4': dict(model='tiny_d16', n_utt=6, beam=4, window=16, plan='small', seed=3, cap=6, seq_len=200, pool=0, scale=6.0),
    'small10': dict(model='tiny_d16', n_utt=6, beam=10, window=16, plan='small', seed=3, cap=6, seq_len=200, pool=0, scale=6.0),
    'deep': dict(model='toy_d2_depth2', n_utt=3, beam=3, window=12, plan='medium', seed=4, cap=6, seq_len=120, pool=0, scale=4.0),
    'embedded': dict(model='tracker_d64_h300', n_utt=3, beam=2, window=16, plan='medium', seed=4, cap=6, seq_len=120, pool=0, scale=1.0),
    'one_launch': dict(model='tracker_d256', n_utt=3, beam=3, window=12, plan='short', seed=0, cap=6, seq_len=60, pool=0, scale=1.0),
    'limits_only': dict(model='tracker_d256', n_utt=3, beam=3, window=12, plan='limits_only', seed=0, cap=6, seq_len=60, pool=0, scale=1.0),
}


def kind_of(spec):
  return spec if isinstance(spec, str) else spec[0]


def _none(n_utt):
  return ('none',) * n_utt


# ---- plans

def _soft(rng, n):
  v = rng.random(n)
  v[v == 0.0] = 0.5
  return ('soft', tuple(float(x) for x in v))


def _refusal(ops, op, wants, tables=None, pending=False):
  """A refusal and the push that has to follow it."""
  ops.append(op)
  ops.append(('push', tuple(wants), tuple(tables) if tables else _none(len(wants)), None, pending))


def _body(rng, n_utt, window, cap, n_ops, limits, fresh, refusals=REFUSALS):
  """n_ops random operations.  limits: the slots' limits when the body begins; fresh: the slots known to have received
  nothing (with and without the policy operations: a slot is fresh from a restart to its next push, prime or move)."""
  limits, fresh = list(limits), set(fresh)
  ops = []
  todo = [r for r in refusals if r != 'prime_long']   # (prime_long needs a fresh slot: drawn where one exists)

  def tables_for(wants):
    out = []
    for u in range(n_utt):
      r = rng.random()
      if wants[u] == 0 or r < 0.2:
        out.append('none')
      elif r < 0.28:
        out.append('nan')
      elif r < 0.36:
        out.append('p0')
      elif r < 0.68 or limits[u] == 1:   # (b = 1 under limit 1 empties the beam: only where the script wants it)
        out.append(_soft(rng, window))
      else:
        out.append(('hard', int(rng.integers(0, 7))))
    return tuple(out)

  def wants_some():
    w = [0 if rng.random() < 0.35 else int(rng.integers(1, 5)) for _ in range(n_utt)]
    if not any(w):
      w[int(rng.integers(0, n_utt))] = 2
    return tuple(w)

  while len(ops) < n_ops:
    r = rng.random()
    if r < 0.40:
      wants = wants_some()
      ops.append(('push', wants, tables_for(wants) if rng.random() < 0.7 else _none(n_utt)))
      fresh -= {u for u in range(n_utt) if wants[u]}
    elif r < 0.45:
      ops.append(('push', tuple('fill' if u == int(rng.integers(0, n_utt)) else int(rng.integers(0, 3)) for u in range(n_utt)),
                  _none(n_utt)))
      fresh.clear()
    elif r < 0.50:
      ops.append(('commit', None))
    elif r < 0.62:
      ops.append(('commit', tuple(int(rng.choice([-1, 0, 2, 3, 5, 8, 2 * window])) for _ in range(n_utt))))
    elif r < 0.70:
      slots = tuple(u for u in range(n_utt) if rng.random() < 0.3) or (int(rng.integers(0, n_utt)),)
      ops.append(('restart', slots))
      fresh |= set(slots)
    elif r < 0.75:
      if fresh:
        slots = [u for u in sorted(fresh) if rng.random() < 0.7] or [min(fresh)]
        ops.append(('prime', {u: (('truth', 'greedy')[int(rng.integers(0, 2))], int(rng.integers(2, cap + 1))) for u in slots}))
        fresh -= set(slots)
    elif r < 0.84:
      limits = [int(rng.choice([0, 1, 2, 3, cap])) if rng.random() < 0.5 else limits[u] for u in range(n_utt)]
      ops.append(('limits', tuple(limits)))
    elif r < 0.93:
      mode = ('query', 'all', 'subset')[int(rng.integers(0, 3))]
      ops.append(('retire', mode, int(rng.integers(0, 1 << 30))))
    elif r < 0.96:
      src, dst = (int(v) for v in rng.choice(n_utt, 2, replace=False))
      ops.append(('move', src, dst))
      fresh -= {src, dst}
    elif todo or fresh:
      what = todo.pop(0) if todo else 'prime_long'
      u = int(rng.integers(0, n_utt))
      wants = wants_some()
      if what == 'push':
        _refusal(ops, ('refuse', 'push', u, 1), [2 if v == u else 0 for v in range(n_utt)])
      elif what == 'prime_received':
        busy = [v for v in range(n_utt) if v not in fresh]
        ops.append(('push', tuple(1 if v == busy[0] else 0 for v in range(n_utt)), _none(n_utt)))   # (it has received)
        _refusal(ops, ('refuse', 'prime_received', busy[0]), [1 if v == busy[0] else 0 for v in range(n_utt)])
      elif what == 'prime_long':
        u = min(fresh)
        _refusal(ops, ('refuse', 'prime_long', u), [2 if v == u else 0 for v in range(n_utt)])
        fresh.discard(u)
      elif what == 'bias_length':
        _refusal(ops, ('refuse', 'bias_length', wants), wants)
      elif what == 'bias_push_long':
        _refusal(ops, ('refuse', 'bias_push_long', u, 2), [1 if v == u else 0 for v in range(n_utt)])
      elif what == 'bias_prime':
        ops.append(('restart', (u,)))
        _refusal(ops, ('refuse', 'bias_prime', u), [3 if v == u else wants[v] for v in range(n_utt)])
      elif what == 'limits_range':
        _refusal(ops, ('refuse', 'limits_range', tuple(4097 if v == u else 2 for v in range(n_utt))), wants)
      elif what == 'bias_value':
        tabs = tuple(_soft(rng, window) if wants[v] else 'none' for v in range(n_utt))
        _refusal(ops, ('refuse', 'bias_value', wants, tabs), wants, tabs, pending=True)
      else:
        _refusal(ops, ('refuse', what, wants), wants)
      fresh -= {v for v in range(n_utt) if ops[-1][1][v]}
  return ops


def _three_slot_prologue(rng, window, cap, tables=True):
  """About 85 frames over three slots: every new operation, both contradictions, a prefix above its bound, a move
  between slots of different limits, every refusal of a table.  tables False: the same without tables and without the
  refusals of tables (a persistent session takes none)."""
  soft = lambda: _soft(rng, window)   # pylint: disable=unnecessary-lambda-assignment
  t = (lambda *specs: tuple(specs)) if tables else (lambda *specs: _none(3))   # pylint: disable=unnecessary-lambda-assignment
  ops = [
      ('limits', (1, 2, cap)),
      ('push', (3, 3, 3), t(soft(), ('hard', 1), 'p0')),
      ('push', (2, 0, 2), t('nan', 'none', ('hard', 3))),              # rows behind a silent slot
      ('limits', (3, 1, cap)),                                          # raised 1 -> 3; lowered 2 -> 1 below a live K
      ('push', (3, 2, 3), t(('hard', 2), soft(), 'none')),
      ('commit', (0, 2, 2)),                                            # a positive horizon between biased pushes; slot 0: all
      ('retire', 'query', 0),
      ('retire', 'all', 0),
      ('push', (3, 2, 2), t(soft(), 'none', ('hard', 5))),              # a cluster opens again under limit 3
      ('limits', (3, 0, cap)),                                          # a binding bound lifted from live clusters
      ('push', (2, 3, 0), t(soft(), ('hard', 2), 'none')),              # ... an unbounded slot beside a bounded one
      ('move', 0, 2),                                                   # limit 3 -> a slot of limit cap
      ('push', (1, 0, 2), t(soft(), 'none', ('hard', 4))),              # the moved utterance, behind a silent slot
      ('commit', None),
      ('push', (0, 2, 0), t('none', soft(), 'none')),                   # the unbounded slot goes on (steered where it must be)
      ('limits', (3, 3, cap)),                                          # ... and is bounded again
  ]
  if tables:
    _refusal(ops, ('refuse', 'bias_length', (2, 1, 1)), (2, 1, 1))
    _refusal(ops, ('refuse', 'bias_push_long', 2, 1), (0, 0, 1))
    stays = (soft(), 'none', soft())                                    # (the table that stays pending behind the refusal)
    _refusal(ops, ('refuse', 'bias_value', (1, 0, 2), stays), (1, 0, 2), stays, pending=True)
  _refusal(ops, ('refuse', 'limits_range', (2, 4097, 0)), (1, 1, 0))
  ops += [
      ('restart', (0, 2)),
      ('limits', (1, 1, 2)),
      ('push', (2, 1, 0), t('none', soft(), 'none')),
      ('push', (1, 1, 1), t(('raw', (1.0,)), soft(), ('raw', (0.0,)))),   # b = 1 under limit 1; b = 0 at a first frame
      ('commit', (0, 0, 0)),
      ('restart', (0, 2)),
      ('limits', (3, 1, 1)),
      ('push', (2, 1, 2), t(soft(), 'none', soft())),                   # the dead slots live again
      ('restart', (2,)),
  ]
  if tables:
    _refusal(ops, ('refuse', 'bias_prime', 2), (0, 0, 2))
    ops.append(('restart', (2,)))
  ops += [
      ('prime', {2: ('truth', cap)}),                                   # a prefix of more clusters than its limit of 1
      ('push', (1, 1, 4), t(soft(), 'none', ('hard', 6))),
      ('commit', (3, 3, 3)),
      ('retire', 'subset', 5),
      ('push', (2, 2, 2), t('none', 'p0', soft())),
  ]
  return ops


def small_plan(n_utt, window, cap, seed):
  """Six slots: the three-slot script on slots 0 - 2 with slots 3 - 5 alongside, session_walk's refusals and its
  non-finite frame, a slot at limit == cap that is fed until it sits at the cap, then the body."""
  assert n_utt == 6
  rng = np.random.default_rng(seed)
  soft = lambda: _soft(rng, window)   # pylint: disable=unnecessary-lambda-assignment
  side_w = ((2, 4, 1), (3, 0, 2), (1, 3, 4), (0, 2, 3), (4, 1, 0), (2, 2, 2))
  side_t = (lambda: (soft(), 'none', ('hard', 2)), lambda: ('p0', 'none', soft()), lambda: ('none', ('hard', 0), 'nan'))
  pro, k = [], 0
  for op in _three_slot_prologue(rng, window, cap):
    if op[0] == 'push' and len(op) == 5:   # (the push behind a refusal: the slots the refusal named, no others)
      pro.append(('push', op[1] + (0, 0, 0), op[2] + _none(3)) + op[3:])
    elif op[0] == 'push':
      w = side_w[k % len(side_w)]
      tabs = tuple(s if w[i] else 'none' for i, s in enumerate(side_t[k % len(side_t)]()))
      pro.append(('push', op[1] + w, op[2] + (tabs if any(kind_of(s) != 'none' for s in op[2]) else _none(3))) + op[3:])
      k += 1
    elif op[0] == 'limits':
      pro.append(('limits', op[1] + ((cap, 0, 3) if k < 4 else (cap, 2, 0))))
    elif op[0] == 'commit':
      pro.append(('commit', None if op[1] is None else op[1] + (4, -1, 2)))
    elif op[0] == 'refuse' and op[1] in ('bias_length', 'bias_value'):
      pro.append(op[:2] + (op[2] + (0, 0, 0),) + tuple(x + _none(3) for x in op[3:]))
    elif op[0] == 'refuse' and op[1] == 'limits_range':
      pro.append(('refuse', 'limits_range', op[2] + (cap, 0, 3)))
    else:
      pro.append(op)
  pro += [
      ('limits', (2, 1, 3, cap, 0, cap)),
      ('push', (0, 0, 0, 'fill', 2, 2), _none(6)),                      # slot 3 holds the whole window
      ('refuse', 'push', 5, 1),
      ('push', (0, 0, 0, 0, 0, 1), _none(6)),
      ('commit', (4, 4, 4, 6, 4, 4)),
      ('push', (2, 0, 2, 4, 0, 3), ('none', 'none', soft(), ('hard', 3), 'none', soft()), 2),   # a non-finite frame
      ('refuse', 'prime_received', 3),
      ('push', (0, 0, 0, 2, 0, 0), _none(6)),
      ('commit', None),
      ('restart', (2, 4)),
      ('refuse', 'prime_long', 4),
      ('push', (0, 0, 0, 0, 2, 0), _none(6)),
      ('prime', {2: ('greedy', 5)}),
      ('move', 5, 4),                                                   # limit cap -> an unbounded slot
      ('push', (1, 0, 2, 4, 3, 0), (soft(), 'none', 'none', 'none', ('hard', 1), 'none')),
  ]
  # slot 3, bounded by the cap itself, walks through more speakers than that: it reaches K == cap and stays there
  pro += [('restart', (3,))]
  for k in range(9):
    # (forced changes of speaker first, so that it gets there soon: this model merges what lies close)
    own = ('raw', (1.0, NAN, 1.0)) if k < 4 else ('hard', k) if k % 2 else 'none'
    pro += [('push', (k % 2, 0, 1, 4, 0, (k + 1) % 2), ('none', 'none', soft() if k % 3 == 0 else 'none', own, 'none', 'nan')),
            ('commit', (-1, 3, -1, 4, -1, 5))]
  limits = (2, 1, 3, cap, 0, cap)
  body = _body(rng, n_utt, window, cap, 48, limits, fresh=())
  epi = [
      ('commit', (3, 3, 3, 3, 3, 3)),
      ('retire', 'all', 0),
      ('push', (3, 0, 2, 0, 1, 2), _none(6)),
      ('restart', tuple(range(n_utt))),
      ('push', (1, 2, 0, 3, 0, 1), (soft(), ('hard', 2), 'none', 'nan', 'none', 'p0')),
      ('commit', None),
  ]
  return tuple(pro + body + epi)


def medium_plan(n_utt, window, cap, seed):
  """Three slots, about sixty operations: the script, session_walk's three refusals, a body."""
  assert n_utt == 3
  rng = np.random.default_rng(seed)
  pro = _three_slot_prologue(rng, window, cap)
  pro += [
      ('push', ('fill', 1, 0), _none(3)),
      ('refuse', 'push', 0, 2),
      ('push', (0, 1, 1), _none(3)),
      ('refuse', 'prime_received', 0),
      ('push', (0, 1, 0), _none(3)),
      ('commit', (3, 2, -1)),
      ('push', (2, 1, 0), _none(3)),                                    # (the pruned beams widen again)
      ('restart', (2,)),
      ('refuse', 'prime_long', 2),
      ('push', (1, 0, 2), _none(3)),
  ]
  body = _body(rng, n_utt, window, cap, 14, (1, 1, 2), fresh=(), refusals=())
  return tuple(pro + body + [('commit', (0, 0, 0)), ('push', (2, 1, 2), _none(3)), ('restart', (0, 1, 2))])


def _short_tail():
  """session_walk's three refusals behind the script, each with its push."""
  ops = []
  _refusal(ops, ('refuse', 'push', 0, 1), (1, 0, 0))
  _refusal(ops, ('refuse', 'prime_received', 1), (0, 1, 0))
  ops.append(('restart', (2,)))
  _refusal(ops, ('refuse', 'prime_long', 2), (0, 0, 1))
  return ops


def short_plan(n_utt, window, cap, seed):
  """The one-launch shape: the script and session_walk's refusals, nothing drawn."""
  assert n_utt == 3
  return tuple(_three_slot_prologue(np.random.default_rng(seed), window, cap) + _short_tail())


def limits_only_plan(n_utt, window, cap, seed):
  """The script without tables, for the persistent path: its one refusal of a table is bias_push_persistent."""
  assert n_utt == 3
  ops = _three_slot_prologue(np.random.default_rng(seed), window, cap, tables=False)
  at = ops.index(('limits', (3, 3, cap)))   # (behind the stretch in which slot 1 is unbounded: nothing steers here)
  tail = []
  _refusal(tail, ('refuse', 'bias_push_persistent', (2, 1, 1)), (2, 1, 1))
  return tuple(ops[:at + 1] + tail + ops[at + 1:] + _short_tail())


PLANS = {'small': small_plan, 'medium': medium_plan, 'short': short_plan, 'limits_only': limits_only_plan}


def strip(plan):
  """The plan without the two rules: a session_walk plan."""
  out = []
  for op in plan:
    if op[0] == 'push':
      out.append(('push', op[1]) + ((op[3],) if len(op) > 3 and op[3] is not None else ()))
    elif op[0] in ('limits', 'retire', 'move') or (op[0] == 'refuse' and op[1] not in ('push', 'prime_received', 'prime_long')):
      continue
    else:
      out.append(op)
  return tuple(out)


def retable(plan, kind):
  """The plan with every table that is not 'none' replaced by `kind` (scripted contradictions included)."""
  return tuple(op[:2] + (tuple(s if kind_of(s) == 'none' else kind for s in op[2]),) + op[3:] if op[0] == 'push' else
               (op[:3] + (tuple(s if kind_of(s) == 'none' else kind for s in op[3]),) if op[:2] == ('refuse', 'bias_value') else op)
               for op in plan)


# ---- the reference

def _clone(ref, limit=None):
  """A second bias_ref.Session in the state of `ref` (limit: another slot's)."""
  new = bias_ref.Session(ref.model, ref.beam_size, ref.limit if limit is None else limit)
  new.beam = [h.copy() for h in ref.beam]
  new.received, new.committed = ref.received, ref.committed
  new.final, new.history, new.gone, new.retired = list(ref.final), list(ref.history), list(ref.gone), list(ref.retired)
  return new


def _opened(h):
  """The hypothesis' last frame opened a cluster."""
  return bool(h.trace) and h.last == len(h.means) - 1 and h.counts[h.last] == 1


class _Life(sw._Life):   # pylint: disable=protected-access
  """One utterance: from uis_stream_begin or a restart to the next restart; a move takes it to another slot."""

  def __init__(self, model, beam, slot, seq, truth, limit):
    super().__init__(model, beam, slot, seq, truth)
    self.ref = bias_ref.Session(model, beam, int(limit))
    self.raw_final = []     # the committed labels as the device handed them out
    self.tables = []        # the table entry of every frame received (NaN: none)
    self.touched = set()    # 'commit', 'retire', 'move', 'limits': what keeps it from being an offline decode
    self.limit0 = int(limit)

  def prime(self, source, n):
    limit = self.ref.limit
    frames, labels, bits = super().prime(source, n)
    start = self.ref.beam[0]
    self.ref = bias_ref.Session(self.model, self.beam, limit, start)
    self.tables.extend([NAN] * n)
    return frames, labels, bits

  def most(self):
    return max([len(h.means) for h in self.ref.beam] or [0])

  def column(self):
    ref, beam, final = self.ref, self.beam, self.raw_final
    inf = sw._bits(np.full(beam, np.inf)).tolist()   # pylint: disable=protected-access
    if ref.received == 0:
      col = {'labels': [], 'scores': 0, 'beam': inf, 'overflow': 0, 'rows': [], 'nb_scores': inf, 'counts': 0, 'stable': 0}
    elif not ref.beam:
      col = {'labels': list(final) + [-1] * ref.have, 'scores': inf[0], 'beam': inf, 'overflow': 0, 'rows': [],
             'nb_scores': inf, 'counts': 0, 'stable': ref.committed}
    else:
      padded = sw._bits(primed_ref.padded_beam(ref.scores(), beam)).tolist()   # pylint: disable=protected-access
      rows = ref.rows().tolist()
      col = {'labels': list(final) + rows[0], 'scores': padded[0], 'beam': padded, 'overflow': 0,
             'rows': [list(final) + r for r in rows], 'nb_scores': padded, 'counts': len(ref.beam),
             'stable': ref.committed + ref.stable()}
    col['received'], col['committed'], col['limit'] = ref.have, ref.committed, int(ref.limit or 0)
    return col


def make_pools(model_name, n_utt, seq_len, pool=0, scale=1.0):
  """POOL_SEQS speaker walks per slot, 6 or 7 speakers in segments of 2 to 4 frames, with their speaker ids."""
  dim = int(golden_util.load_case(model_name)['params']['observation_dim'])
  out = []
  for u in range(n_utt):
    seqs = []
    for k in range(sw.POOL_SEQS):
      n_spk, seg = 6 + (u + k) % 2, 2 + (u + 2 * k + pool) % 3
      seq = retire_ref.speaker_walk(8000 + 1000 * pool + 100 * u + k, dim, n_spk, seg, seq_len, scale=scale)
      seqs.append((seq, (np.arange(seq_len) // seg) % n_spk))
    out.append(seqs)
  return out


def _table(spec, n, p0):
  kind = kind_of(spec)
  if kind in ('none', 'nan'):
    return np.full(n, np.nan)
  if kind == 'p0':
    return np.full(n, p0, dtype=np.float64)
  if kind == 'soft':
    return np.array(spec[1][:n], dtype=np.float64)
  if kind == 'hard':
    return bias_ref.pattern(int(spec[1]), n)
  assert kind == 'raw', spec
  return np.array((list(spec[1]) + [np.nan] * n)[:n], dtype=np.float64)


def trace(params, pools, beam, max_frames, plan, max_clusters, shadows=False):
  """Run `plan` on the reference.  Returns dict(steps, lives, ...): steps[i] = dict(op, kind, call, result, snap, before,
  aux) as session_walk.trace's, aux: what facts() reads (K and life of every slot afterwards; with `shadows` also what
  a one-step shadow without the bound, and the same push without its table, would have given)."""
  oracle.lib()
  model = primed_ref.Model(params)
  p0 = float(params['transition_bias'])
  n_utt, cap = len(pools), int(max_clusters)
  nxt = [0] * n_utt
  lives = []
  limits = [0] * n_utt

  def begin(u):
    seq, truth = pools[u][nxt[u] % len(pools[u])]
    nxt[u] += 1
    lives.append(_Life(model, beam, u, seq, truth, limits[u]))
    return lives[-1]

  slots = [begin(u) for u in range(n_utt)]
  log_len = max_frames + 2
  steps = []
  state = {'snap': [s.column() for s in slots]}

  def record(op, kind, call, result, aux=None):
    before = state['snap']
    state['snap'] = [s.column() for s in slots]
    for s in slots:
      assert s.most() <= cap, (len(steps), op, s.slot, 'the reference passes the cap')
    aux = dict(aux or {})
    aux.update(K=[s.ref.K() for s in slots], life=[lives.index(s) for s in slots], most=[s.most() for s in slots],
               stream_labels=[s.ref.labels() for s in slots])   # (in stream ids: what uisrnn_amd.OnlineSession hands out)
    steps.append({'op': op, 'kind': kind, 'call': call, 'result': result, 'snap': state['snap'], 'before': before, 'aux': aux})

  def sizes(wants):
    out = []
    for u, s in enumerate(slots):
      room, left = max_frames - s.ref.have, len(s.seq) - s.pos
      out.append(min(room, left) if wants[u] == 'fill' else min(int(wants[u]), room, left))
    return out

  def peek(wants):
    return [np.array(s.seq[s.pos:s.pos + n], dtype=np.float64) if n else None for s, n in zip(slots, sizes(wants))]

  def whole_table(chunks, tables):
    if all(kind_of(tables[u]) == 'none' for u in range(n_utt) if chunks[u] is not None):
      return None, [None] * n_utt
    per = [None if c is None else _table(tables[u], len(c), p0) for u, c in enumerate(chunks)]
    return np.concatenate([t for t in per if t is not None]), per

  def commit(op, horizons):
    nonlocal log_len
    have = [s.ref.have for s in slots]
    most = max(s.ref.received for s in slots)
    out = []
    for u, s in enumerate(slots):
      ids, dropped = s.ref.commit(None if horizons is None else horizons[u])
      raw = [retire_ref.to_local(g, s.ref.gone) for g in ids]
      s.raw_final.extend(raw)
      s.events.append((len(steps), 'commit', raw))
      if raw or dropped:
        s.touched.add('commit')
      out.append((raw, dropped))
    line, grew = None, False
    if sum(have):
      if most + max_frames + 2 > log_len:
        log_len, grew = max(2 * log_len, most + max_frames + 2), True
      line = {'window_frames': sum(have), 'committed': sum(len(o[0]) for o in out), 'prior_table_entries': log_len}
    record(op, 'commit_none' if horizons is None else 'commit_h', {'horizons': horizons},
           {'labels': [o[0] for o in out], 'dropped': [o[1] for o in out], 'line': line, 'have': have}, {'grew': grew})

  def retire(op, which=None, picks=None):
    able = [s.ref.retirable() for s in slots]
    if picks is None:
      picks = [able[u] if which is None or which[u] else [] for u in range(n_utt)]
    k_before = [s.ref.K() for s in slots]
    for s, pick in zip(slots, picks):
      s.ref.retire(pick)
      if pick:
        s.touched.add('retire')
    call = {'which': which, 'clusters': None if which is not None or op[1] == 'all' else [p or None for p in picks]}
    record(op, 'retire', call, {'retired': [list(p) for p in picks], 'K': [s.ref.K() for s in slots], 'retirable': able},
           {'K_before': k_before})

  def restart(op, which):
    before, result = state['snap'], {}
    for u in which:
      col = before[u]
      result[u] = {'labels': col['labels'], 'window': col['labels'][col['committed']:], 'score': col['scores'], 'overflow': 0}
      slots[u].end, slots[u].end_col = (col['labels'], col['scores']), col
      slots[u] = begin(u)
    record(op, 'restart', {'which': [u in which for u in range(n_utt)]}, result)

  for op in plan:
    kind = op[0]
    if kind == 'push':
      wants = op[1]
      if len(op) > 2 and isinstance(op[2], tuple):
        tables, bad = op[2], op[3] if len(op) > 3 else None
      else:   # session_walk's form: ('push', wants[, bad])
        tables, bad = _none(n_utt), op[2] if len(op) > 2 else None
      pending = bool(op[4]) if len(op) > 4 else False
      n_new = sizes(wants)
      # the reference steers the unbounded slots away from the cap
      tight = [u for u, s in enumerate(slots) if n_new[u] and limits[u] == 0 and s.most() and s.most() + max(n_new[u], 3) > cap]
      if tight:
        # (a refusal and the push behind it belong together -- a pending table is sized for that push: nothing may
        # come between them.  The plans keep the slots of such a push away from the cap)
        assert not steps or steps[-1]['kind'] != 'refuse', (len(steps), op, 'the reference would steer between a refusal and its push')
        commit(('steer', 'commit'), [2 if u in tight else -1 for u in range(n_utt)])
        retire(('steer', 'retire'), which=[u in tight for u in range(n_utt)])
        still = [u for u in tight if slots[u].most() and slots[u].most() + max(n_new[u], 3) > cap]
        if still:
          restart(('steer', 'restart'), still)
        n_new = sizes(wants)
      # (a frame opens one cluster at the most: an unbounded slot takes no more frames than it has clusters left)
      n_new = [min(n, cap - s.most()) if limits[u] == 0 else n for u, (n, s) in enumerate(zip(n_new, slots))]
      chunks = []
      for u, s in enumerate(slots):
        assert not (bad == u and n_new[u] == 0), 'the non-finite frame was clipped away'
        chunks.append(s.take(n_new[u], bad == u) if n_new[u] else None)
      bias, per = whole_table(chunks, tables)
      aux = {'kinds': [None if c is None else kind_of(tables[u]) for u, c in enumerate(chunks)], 'bound': [], 'changed': {},
             'limits': list(limits), 'first': [s.ref.received == 0 for s in slots], 'tables': per}
      for u, (s, part) in enumerate(zip(slots, chunks)):
        if part is None:
          continue
        tab = per[u] if kind_of(tables[u]) != 'none' else None
        x32 = np.asarray(part, dtype=np.float32)
        plain = zeros = ones = None
        if shadows and tab is not None and kind_of(tables[u]) in ('soft', 'hard', 'raw') and s.ref.beam:
          plain = _clone(s.ref)
          if kind_of(tables[u]) != 'soft':
            zeros = _clone(s.ref) if (tab == 0.0).any() else None
            ones = _clone(s.ref) if (tab == 1.0).any() else None
        with np.errstate(all='ignore'):
          for t in range(len(part)):
            lim = limits[u]
            if shadows and lim and s.ref.beam and any(len(h.means) == lim for h in s.ref.beam):
              free = bias_ref.step(model, s.ref.beam, x32[t:t + 1], beam, None, None if tab is None else [tab[t]])
              if any(_opened(h) and len(h.means) - 1 >= lim for h in free) and u not in aux['bound']:
                aux['bound'].append(u)
            s.ref.push(part[t:t + 1], None if tab is None else tab[t:t + 1])
            assert s.most() <= cap, (len(steps), op, u, 'the reference passes the cap')
          if plain is not None:
            got = s.ref.rows().tolist()[:1]
            plain.push(part)
            ch = {'any': plain.rows().tolist()[:1] != got, 'hard0': False, 'hard1': False}
            for name, other, val in (('hard0', zeros, 0.0), ('hard1', ones, 1.0)):
              if other is not None:
                other.push(part, np.where(tab == val, val, np.nan))
                ch[name] = other.rows().tolist()[:1] != plain.rows().tolist()[:1]
            aux['changed'][u] = ch
        s.given.extend(np.asarray(part, dtype=np.float64))
        s.tables.extend(np.full(len(part), np.nan) if tab is None else tab)
        s.events.append((len(steps), 'push', len(part)))
      record(op, 'push', {'chunks': chunks, 'bias': None if pending else bias, 'pending': pending}, None, aux)
    elif kind == 'commit':
      commit(op, None if op[1] is None else [int(v) for v in op[1]])
    elif kind == 'restart':
      restart(op, list(op[1]))
    elif kind == 'prime':
      chunks, labels, result = [None] * n_utt, [None] * n_utt, {}
      for u, (source, n) in sorted(op[1].items()):
        chunks[u], labels[u], result[u] = slots[u].prime(source, max_frames if n == 'window' else int(n))
      record(op, 'prime', {'chunks': chunks, 'labels': labels}, result)
    elif kind == 'limits':
      old = list(limits)
      for u, v in enumerate(op[1]):
        if int(v) != limits[u] and slots[u].ref.received:
          slots[u].touched.add('limits')
        elif int(v) != limits[u]:
          slots[u].limit0 = int(v)   # (before its first frame: the limit it decodes under from the start)
        limits[u] = int(v)
        slots[u].ref.set_limit(int(v))
      record(op, 'limits', {'limits': list(limits)}, None, {'old': old})
    elif kind == 'retire':
      if op[1] == 'query':
        retire(op, picks=[[] for _ in range(n_utt)])
      elif op[1] == 'all':
        retire(op)
      else:
        rng = np.random.default_rng(op[2])
        retire(op, picks=[[k for k in s.ref.retirable() if rng.random() < 0.5] for s in slots])
    elif kind == 'move':
      src, dst = int(op[1]), int(op[2])
      if slots[src].dead:
        record(op, 'move_refused', {'src': src, 'dst': dst}, INVALID_ARG)
        continue
      before = state['snap']
      aux = {'limits': list(limits), 'have': [c['received'] for c in before]}
      result = {}
      for u in (dst, src):
        col = before[u]
        result[u] = {'labels': col['labels'], 'window': col['labels'][col['committed']:], 'score': col['scores'], 'overflow': 0}
      slots[dst].end, slots[dst].end_col = (before[dst]['labels'], before[dst]['scores']), before[dst]
      moved = slots[src]
      moved.ref = _clone(moved.ref, limits[dst])
      moved.slot = dst
      moved.touched.add('move')
      if moved.ref.received + max_frames + 2 > log_len:   # (an import lengthens the prior tables like a commit)
        log_len = max(2 * log_len, moved.ref.received + max_frames + 2)
      slots[dst] = moved
      slots[src] = begin(src)
      record(op, 'move', {'src': src, 'dst': dst}, result, aux)
    elif kind == 'refuse':
      what = op[1]
      dim = slots[0].seq.shape[1]
      if what in ('push', 'bias_push_long'):
        u = op[2]
        n = max_frames - slots[u].ref.have + int(op[3])
        chunks = [slots[v].seq[slots[v].pos:slots[v].pos + 1] if max_frames > slots[v].ref.have else None for v in range(n_utt)]
        chunks[u] = np.zeros((n, dim))
        bias = np.full(sum(len(c) for c in chunks if c is not None), 0.5) if what == 'bias_push_long' else None
        call, result = {'call': 'push', 'chunks': chunks, 'bias': bias}, INVALID_ARG
      elif what in ('prime_received', 'prime_long', 'bias_prime'):
        u = op[2]
        n = max_frames + 1 if what == 'prime_long' else 2
        assert slots[u].fresh == (what != 'prime_received'), (what, u)
        chunks, labels = [None] * n_utt, [None] * n_utt
        chunks[u], labels[u] = np.tile(slots[u].seq[:1], (n, 1)), np.zeros(n, dtype=np.int32)
        call = {'call': 'prime', 'chunks': chunks, 'labels': labels, 'bias': np.full(n, 0.5) if what == 'bias_prime' else None}
        result = UNSUPPORTED if what == 'bias_prime' else INVALID_ARG
      elif what in ('bias_length', 'bias_push_persistent'):
        chunks = peek(op[2])
        total = sum(len(c) for c in chunks if c is not None)
        assert total >= 2, op
        call = {'call': 'push', 'chunks': chunks, 'bias': np.full(total - (what == 'bias_length'), 0.25)}
        result = INVALID_ARG if what == 'bias_length' else UNSUPPORTED
      elif what == 'limits_range':
        assert 4097 in op[2]
        call, result = {'call': 'limits', 'limits': [int(v) for v in op[2]]}, INVALID_ARG
      elif what == 'bias_value':
        chunks = peek(op[2])
        stays, _ = whole_table(chunks, op[3])
        call, result = {'call': 'frame_bias', 'stays': stays, 'bias': np.array([0.5, 1.5])}, INVALID_ARG
      else:
        raise ValueError(op)
      record(op, 'refuse', call, result)
      assert steps[-1]['snap'] == steps[-1]['before']
    else:
      raise ValueError(op)
  for u, s in enumerate(slots):
    s.end, s.end_col = (state['snap'][u]['labels'], state['snap'][u]['scores']), state['snap'][u]
  return {'steps': steps, 'lives': lives, 'n_utt': n_utt, 'beam': beam, 'max_frames': max_frames, 'cap': cap, 'plan': plan}


def case_plan(name):
  case = CASES[name]
  return PLANS[case['plan']](case['n_utt'], case['window'], case['cap'], case['seed'])


def case_pools(name):
  case = CASES[name]
  return make_pools(case['model'], case['n_utt'], case['seq_len'], case['pool'], case['scale'])


@functools.lru_cache(maxsize=None)
def walk(name, shadows=False):
  """The trace of CASES[name], computed once (shadows: with what facts() needs beyond the trace itself)."""
  case = CASES[name]
  params = golden_util.load_case(case['model'])['params']
  out = trace(params, case_pools(name), case['beam'], case['window'], case_plan(name), case['cap'], shadows)
  out['params'], out['name'] = params, name
  return out


# ---- what a trace reaches

def _pushed(st, u):
  return st['kind'] == 'push' and st['call']['chunks'][u] is not None


def _later(steps, i, u):
  """The steps behind step i while slot u holds the same utterance."""
  life = steps[i]['aux']['life'][u]
  for st in steps[i + 1:]:
    if st['aux']['life'][u] != life:
      return
    yield st


def facts(tr):
  """The conditions of the walk, each a truth value or a count, from a trace made with shadows."""
  steps, n_utt, beam, cap = tr['steps'], tr['n_utt'], tr['beam'], tr['cap']
  f = {}
  f['kinds'] = {k: sum(1 for st in steps if st['kind'] == k) for k in OP_KINDS}
  f['retire_modes'] = {m: sum(1 for st in steps if st['kind'] == 'retire' and st['op'][1] == m) for m in ('query', 'all', 'subset')}
  f['retired'] = sum(len(r) for st in steps if st['kind'] == 'retire' for r in st['result']['retired'])
  f['table_kinds'] = {k: sum(1 for st in steps if st['kind'] == 'push' for x in st['aux']['kinds'] if x == k) for k in TABLE_KINDS}
  f['frames'] = sum(len(life.given) for life in tr['lives'])
  f['operations'] = len(tr['plan'])
  # refusals, each in a session that is not trivial, each followed by a push of the call's slots without a table argument
  ref = {}
  for i, st in enumerate(steps):
    if st['kind'] != 'refuse':
      continue
    busy = any(c['committed'] > 0 for c in st['before']) and any(c['counts'] > 1 for c in st['before'])
    ref[st['op'][1]] = ref.get(st['op'][1], 0) + (1 if busy else 0)
    nxt = steps[i + 1] if i + 1 < len(steps) else None
    follows = nxt is not None and nxt['kind'] == 'push' and nxt['call']['bias'] is None
    if follows and 'chunks' in st['call']:   # the slots the refused call named receive frames (where their window has room)
      follows = all(nxt['call']['chunks'][u] is not None or st['before'][u]['received'] == tr['max_frames']
                    for u, c in enumerate(st['call']['chunks'])
                    if c is not None and (st['call']['call'] != 'push' or st['op'][1] in ('bias_length', 'bias_push_persistent') or u == st['op'][2]))
    f.setdefault('refusals_followed', True)
    f['refusals_followed'] = f['refusals_followed'] and follows
  f['refusals'] = ref
  # the bound bound
  f['bound_steps'] = sum(1 for st in steps if st['kind'] == 'push' and st['aux']['bound'])
  # limit changes with live clusters; a cluster that opens again
  lowered = raised = lifted = reopened = 0
  for i, st in enumerate(steps):
    for u in range(n_utt):
      if st['kind'] == 'limits':
        old, new, k = st['aux']['old'][u], st['call']['limits'][u], st['aux']['K'][u]
        rest = []
        for s in _later(steps, i, u):
          if s['kind'] == 'limits' and s['call']['limits'][u] != new:
            break
          rest.append(s)
        fed = sum(len(s['call']['chunks'][u]) for s in rest if _pushed(s, u) and s['snap'][u]['counts'] > 0)
        if 0 < new < k and fed >= 2:
          assert all(s['aux']['most'][u] <= k for s in rest), (i, u, 'K grew above a lowered limit')
          lowered += 1
        if 0 < old < new and any(s['aux']['K'][u] > old for s in rest):
          raised += 1
        if old > 0 and new == 0 and k >= old and any(s['aux']['K'][u] > k for s in rest):
          lifted += 1   # (the bound bound -- K had reached it -- and without it K grew on)
      elif st['kind'] == 'retire' and st['result']['retired'][u]:
        lim, k0, k1 = st['snap'][u]['limit'], st['aux']['K_before'][u], st['aux']['K'][u]
        if lim and k0 == lim:
          for s in _later(steps, i, u):
            if (s['kind'] == 'limits' and s['call']['limits'][u] != lim) or (s['kind'] == 'retire' and s['result']['retired'][u]):
              break
            if s['aux']['K'][u] > k1:
              reopened += 1
              break
  f['lowered_below_K'], f['raised_and_grew'], f['reopened_after_retirement'] = lowered, raised, reopened
  f['lifted_and_grew'] = lifted
  # a push that gives frames to a bounded and to an unbounded slot
  f['mixed_pushes'] = sum(1 for st in steps if st['kind'] == 'push' and
                          len({st['aux']['limits'][u] > 0 for u in range(n_utt) if _pushed(st, u) and st['snap'][u]['counts'] > 0}) == 2)
  # at the cap: frames received by an utterance while K == cap == its limit
  at_cap = {}
  for i, st in enumerate(steps):
    for u in range(n_utt):
      if i and _pushed(st, u) and st['before'][u]['limit'] == cap and steps[i - 1]['aux']['most'][u] == cap and \
         steps[i - 1]['aux']['life'][u] == st['aux']['life'][u] and st['snap'][u]['counts'] > 0:
        assert st['snap'][u]['overflow'] == 0
        at_cap[st['aux']['life'][u]] = at_cap.get(st['aux']['life'][u], 0) + len(st['call']['chunks'][u])
  f['frames_at_the_cap'] = max(at_cap.values() or [0])
  # a table changed something
  changed = [ch for st in steps if st['kind'] == 'push' for ch in [st['aux']['changed']] if any(c['any'] for c in ch.values())]
  f['table_changed'] = len(changed)
  f['changed_by_0'] = sum(1 for ch in changed if any(c['hard0'] for c in ch.values()))
  f['changed_by_1'] = sum(1 for ch in changed if any(c['hard1'] for c in ch.values()))
  # a move between slots of different limits (and window parities); the moved utterance's rows behind a silent slot's
  moves = parity = behind = 0
  for i, st in enumerate(steps):
    if st['kind'] != 'move':
      continue
    src, dst = st['call']['src'], st['call']['dst']
    if st['aux']['limits'][src] == st['aux']['limits'][dst] or st['aux']['have'][src] == 0:
      continue
    moves += 1
    parity += st['aux']['have'][src] % 2 != st['aux']['have'][dst] % 2
    nxt = next((s for s in _later(steps, i, dst) if s['kind'] == 'push'), None)
    if nxt is not None and _pushed(nxt, dst) and nxt['aux']['kinds'][dst] not in (None, 'none') and not nxt['call']['pending']:
      silent = any(nxt['call']['chunks'][v] is None for v in range(dst))
      shifted = any(nxt['call']['chunks'][v] is not None for v in range(dst))
      behind += silent and shifted
  f['moves_between_limits'], f['moves_between_parities'], f['moved_rows_behind_a_silent_slot'] = moves, parity, behind
  # commit and table order
  between = after_growth = 0
  for u in range(n_utt):
    state, grew = {}, {}
    for st in steps:
      life = st['aux']['life'][u]
      biased = _pushed(st, u) and st['aux']['kinds'][u] not in (None, 'none', 'nan', 'p0')
      if biased:
        between += state.get(life) == 2
        after_growth += bool(grew.get(life))
        state[life], grew[life] = 1, False
      elif st['kind'] == 'commit_h' and st['call']['horizons'][u] > 0 and len(st['result']['labels'][u]) >= 2 and state.get(life):
        state[life] = 2
      if st['kind'].startswith('commit') and st['aux']['grew'] and st['before'][u]['received'] > 0:
        grew[life] = True
  f['commit_between_biased_pushes'], f['biased_push_after_the_tables_grew'] = between, after_growth
  # contradictions: a beam emptied by a table, the slot restarted, a full beam again
  contra = {'b1_under_limit_1': 0, 'b0_at_a_first_frame': 0}
  revived = dict(contra)
  for i, st in enumerate(steps):
    if st['kind'] != 'push':
      continue
    bad = st['op'][3] if len(st['op']) > 3 else None   # (every push of a policy plan carries its tables)
    for u in range(n_utt):
      if not _pushed(st, u) or u == bad or st['snap'][u]['counts'] != 0 or st['aux']['tables'][u] is None:
        continue
      tab = st['aux']['tables'][u]
      if st['aux']['first'][u] and tab[0] == 0.0:
        what = 'b0_at_a_first_frame'
      elif st['aux']['limits'][u] == 1 and (tab == 1.0).any() and st['before'][u]['counts'] > 0:
        what = 'b1_under_limit_1'
      else:
        continue
      contra[what] += 1
      again = False
      for s in steps[i + 1:]:
        again = again or (s['kind'] == 'restart' and s['call']['which'][u])
        if again and s['snap'][u]['counts'] == beam:
          revived[what] += 1
          break
  f['contradictions'], f['revived'] = contra, revived
  # a primed prefix of more clusters than the limit, and at least four frames behind it
  primed = 0
  for i, st in enumerate(steps):
    if st['kind'] != 'prime':
      continue
    for u in st['result']:
      k, lim = st['aux']['K'][u], st['snap'][u]['limit']
      if lim and k > lim:
        rest = list(_later(steps, i, u))
        fed = sum(len(s['call']['chunks'][u]) for s in rest if _pushed(s, u) and s['snap'][u]['limit'] == lim)
        primed += fed >= 4 and all(s['aux']['most'][u] <= k for s in rest if s['snap'][u]['limit'] == lim)
  f['primed_above_the_limit'] = primed
  f['steered'] = sum(1 for st in steps if st['op'][0] == 'steer')
  return f


def offline_lives(tr):
  """The utterances an offline decode can restate: never committed, retired, moved or primed, their limit never
  changed, no non-finite frame."""
  return [life for life in tr['lives'] if life.given and not life.touched and life.prefix is None and not life.bad]
