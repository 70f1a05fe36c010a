"""Model-based walks over a streaming session: plans, and their trace on the CPU reference.  No device, no library.

A PLAN is a deterministic list of operations on an n_utt-slot session, written without knowing what the model will
answer: a scripted prologue that forces the rare states, then a body drawn from np.random.default_rng(seed).

  ('push', wants[, bad])     wants[u]: frames for slot u -- an int (0: the slot is silent, its chunk is None) or 'fill'
                             (as many as fill its window to max_frames).  Never more than the room the window has left
                             or than the slot's sequence still holds: the trace clips.  bad = a slot: the first of its
                             new frames holds +inf in feature 0 (every candidate non-finite: its beam empties)
  ('commit', None)           uis_stream_commit without horizons
  ('commit', horizons)       one int per slot: negative = none for that slot, 0, small, larger than `have`
  ('restart', slots)         the slots end; each goes on with the next sequence of its pool
  ('prime', {slot: (source, length)})   only slots that have received nothing.  source 'truth': the first-appearance
                             form of the synthetic sequence's speaker ids; 'greedy': the reference's own beam-1 labels.
                             length: an int or 'window' (= max_frames)
  ('refuse', 'push', slot, extra)       a push of room + extra frames to that slot (its neighbours get one frame each:
                             the call is all or nothing)
  ('refuse', 'prime_received', slot)    a prime of a slot that has received frames
  ('refuse', 'prime_long', slot)        a prime of max_frames + 1 frames (a slot that has received nothing)

trace() runs a plan on tests/commit_ref.py's Session, one object per slot (prime: a Session started from
tests/primed_ref.py's advance_forced; restart: a new Session), and returns for every operation the call as the device
is to receive it, the result it must give and the snapshot of every slot afterwards.  Nothing in it comes from a device.
facts() says which of the states the walk is meant for a trace reaches; tests/test_session_walk_host.py asserts them.

Outside the model: the cluster cap (max_clusters is chosen so that the reference never gets near it, asserted here),
look_ahead > 1 and test_iteration > 1 (sessions have neither).
"""

import functools

import numpy as np

import commit_ref
import golden_util
import primed_ref
from oracle import oracle
from uisrnn_amd import synth

INVALID_ARG = -1   # UIS_ERR_INVALID_ARG of include/uisrnn_hip.h: what each of the three refused calls returns
PER_UTT = ('labels', 'scores', 'beam', 'overflow', 'rows', 'nb_scores', 'counts', 'stable')   # test_gpu_restart.PER_UTT
KINDS = ('push', 'commit_none', 'commit_h', 'restart', 'prime', 'refuse')
PAIRS = (('push', 'commit'), ('commit', 'commit'), ('commit_h', 'restart'), ('restart', 'prime'), ('prime', 'commit'),
         ('prime', 'restart'), ('restart', 'restart'), ('restart', 'push'), ('commit', 'push'))

# name: the model (a tests/golden case), slots x beam x window, the plan, max_clusters, frames per pool sequence
CASES = {
    'small4': dict(model='tiny_d16', n_utt=6, beam=4, window=16, plan='small', seed=11, cap=16, seq_len=160),
    'small10': dict(model='tiny_d16', n_utt=6, beam=10, window=16, plan='small', seed=11, cap=16, seq_len=160),
    'deep': dict(model='toy_d2_depth2', n_utt=3, beam=3, window=12, plan='medium', seed=5, cap=16, seq_len=40),
    'embedded': dict(model='tracker_d64_h300', n_utt=3, beam=2, window=16, plan='medium', seed=5, cap=16, seq_len=48),
    'one_launch': dict(model='tracker_d256', n_utt=3, beam=3, window=12, plan='short', seed=0, cap=16, seq_len=24),
}
POOL_SEQS = 6   # sequences per slot; a restart takes the next one (and starts over after the last)


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def first_appearance(ids):
  names = {}
  return [names.setdefault(int(i), len(names)) for i in ids]


# ---- plans

def _body(rng, n_utt, max_frames, n_ops, keep, fresh):
  """n_ops random operations.  keep: a slot the body never restarts (it is the one that has to outlive the prior
  tables); fresh: the slots that have received nothing when the body begins (known without the model: a slot stays
  fresh until a push gives it a frame or it is primed)."""
  fresh = set(fresh)
  ops = []
  others = [u for u in range(n_utt) if u != keep]
  for _ in range(n_ops):
    r = rng.random()
    if r < 0.50 or (0.85 <= r < 0.93 and not fresh):
      wants = tuple(0 if rng.random() < 0.35 else int(rng.integers(1, 5)) for _ in range(n_utt))
      ops.append(('push', wants))
      fresh -= {u for u in range(n_utt) if wants[u]}
    elif r < 0.60:
      ops.append(('commit', None))
    elif r < 0.75:
      ops.append(('commit', tuple(int(rng.choice([-1, 0, 2, 3, 5, 8, 2 * max_frames])) for _ in range(n_utt))))
    elif r < 0.85:
      which = rng.integers(0, 4)   # nothing, one slot, a non-contiguous subset, several
      slots = ((), (int(rng.choice(others)),), tuple(others[::2]), tuple(others[1:]))[which]
      ops.append(('restart', slots))
      fresh |= set(slots)
    elif r < 0.93:
      slots = [u for u in sorted(fresh) if rng.random() < 0.7] or [min(fresh)]
      ops.append(('prime', {u: (('truth', 'greedy')[int(rng.integers(0, 2))], int(rng.integers(1, max_frames // 2 + 1)))
                            for u in slots}))
      fresh -= set(slots)
    else:
      ops.append(('push', tuple('fill' if u == int(rng.integers(0, n_utt)) else int(rng.integers(0, 3)) for u in range(n_utt))))
      fresh.clear()   # (a 'fill' or a positive count: conservatively, nobody is known to be fresh any more)
  return ops


def small_plan(n_utt, max_frames, seed):
  """Six slots.  The prologue: a prime of the whole window and the commit that empties it; commits with every kind of
  horizon; restarts of an emptied window, of a slot that never received a frame, of the same slot twice; a prime of a
  just-restarted slot between odd and even neighbours; a push that fills a window to the brim and the one that is
  refused behind it; a non-finite frame, the commit and the restart of the slot it killed; both refused primes."""
  assert n_utt == 6
  pro = [
      ('push', (3, 5, 2, 4, 0, 1)),
      ('prime', {4: ('truth', 'window')}),                    # exactly max_frames frames
      ('commit', None),                                       # ... all of them stable: the window empties
      ('commit', (-1, 0, 2 * max_frames, 2, 3, -1)),          # have 0 (slot 4); a horizon larger than have (slot 2)
      ('restart', (4,)),                                      # an empty window behind a commit, a committed part
      ('restart', (4, 5)),                                    # ... again: a slot that never received a frame
      ('prime', {4: ('greedy', 5)}),                          # a just-restarted slot; its neighbours are odd and even
      ('restart', (4,)),
      ('push', (2, 2, 2, 'fill', 3, 0)),                      # slot 3 holds max_frames
      ('refuse', 'push', 3, 1),
      ('push', (0, 0, 2, 0, 0, 3), 2),                        # slot 2 loses its beam
      ('commit', None),
      ('refuse', 'prime_received', 0),
      ('restart', (2, 5)),                                    # an emptied beam
      ('refuse', 'prime_long', 5),
      ('prime', {5: ('truth', 3), 2: ('greedy', 7)}),
      ('commit', (4, 4, 4, 4, 4, 4)),
      ('push', (5, 4, 5, 3, 5, 4)),
      ('commit', (0, 2, -1, 0, 8, 3)),                        # hypotheses leave the beam
      ('restart', (1, 3)),                                    # right behind a commit with horizons
      ('push', (4, 3, 4, 4, 4, 4)),
      ('push', (4, 3, 4, 4, 4, 4)),                           # the pruned beams are full again
      ('commit', (3, -1, 5, -1, 2, 0)),
  ]
  rng = np.random.default_rng(seed)
  body = _body(rng, n_utt, max_frames, 80, keep=0, fresh=())
  epi = [
      ('commit', (3, 3, 3, 3, 3, 3)),
      ('push', (3, 0, 2, 0, 1, 2), 4),                        # a second non-finite frame, late in the walk
      ('commit', (0, 0, 0, 0, 0, 0)),
      ('restart', tuple(range(n_utt))),
      ('push', (1, 2, 0, 3, 0, 1)),
      ('commit', None),
  ]
  return tuple(pro + body + epi)


def medium_plan(n_utt, max_frames, seed):
  """Three slots, about sixty operations: the same kinds on the other model shapes."""
  assert n_utt == 3
  pro = [
      ('push', (3, 0, 4)),
      ('prime', {1: ('truth', 'window')}),
      ('commit', None),
      ('commit', (0, -1, 2 * max_frames)),
      ('restart', (1,)),
      ('restart', (1,)),
      ('prime', {1: ('greedy', 4)}),
      ('restart', (1,)),
      ('prime', {1: ('truth', 5)}),
      ('push', ('fill', 2, 1)),
      ('refuse', 'push', 0, 2),
      ('commit', (3, 2, -1)),
      ('push', (0, 2, 2), 2),
      ('commit', None),
      ('refuse', 'prime_received', 0),
      ('restart', (2,)),
      ('refuse', 'prime_long', 2),
      ('prime', {2: ('truth', 3)}),
      ('push', (3, 3, 4)),
      ('commit', (2, 0, 5)),
      ('restart', (0, 2)),
  ]
  rng = np.random.default_rng(seed)
  return tuple(pro + _body(rng, n_utt, max_frames, 36, keep=1, fresh=(0, 2)) +
               [('commit', (0, 0, 0)), ('push', (2, 1, 2)), ('push', (1, 1, 2)), ('restart', (0, 1, 2))])


def short_plan(n_utt, max_frames, seed):
  """The one-launch shape, whose reference costs a sixth of a second per frame: at most 90 frames, all scripted."""
  del max_frames, seed
  assert n_utt == 3
  return (
      ('prime', {0: ('truth', 3)}),
      ('push', (4, 5, 0)),
      ('push', (3, 2, 4)),
      ('commit', (2, -1, 20)),
      ('restart', (0,)),
      ('prime', {0: ('greedy', 4)}),
      ('refuse', 'push', 1, 1),
      ('push', (4, 4, 5)),
      ('commit', None),
      ('push', (2, 0, 3)),
      ('restart', (1, 2)),
      ('push', (0, 4, 2)),
      ('commit', (0, 3, -1)),
      ('push', (5, 2, 4)),
      ('commit', (4, 0, 1)),
      ('restart', ()),
      ('push', (1, 1, 1)),
  )


PLANS = {'small': small_plan, 'medium': medium_plan, 'short': short_plan}


# ---- the reference

class _Life:
  """One utterance of one slot: from uis_stream_begin or a restart to the next restart (or the end of the walk)."""

  def __init__(self, model, beam, slot, seq, truth):
    self.model, self.beam, self.slot, self.seq, self.truth = model, beam, slot, seq, truth
    self.ref = commit_ref.Session(model, beam)
    self.pos = 0            # frames of the sequence used up
    self.given = []         # the frames as the device received them (a non-finite one included)
    self.prefix = None      # the labels it was primed with
    self.bad = False        # it received a non-finite frame
    self.end = None         # (labels, score bits) handed out at its restart, or read at the end of the walk
    self.events = []        # (step, 'push', frames) / (step, 'commit', labels handed out), in order

  @property
  def fresh(self):
    return self.ref.received == 0

  @property
  def dead(self):
    return self.ref.received > 0 and not self.ref.beam

  @property
  def pruned(self):
    return any(h.cut > h.stable for h in self.ref.history)

  def take(self, n, bad=False):
    part = np.array(self.seq[self.pos:self.pos + n], dtype=np.float64)
    assert len(part) == n
    if bad:
      part[0, 0] = np.inf
      self.bad = True
    self.pos += n
    return part

  def push(self, part):
    with np.errstate(all='ignore'):
      self.ref.push(part)
    self.given.extend(np.asarray(part, dtype=np.float64))

  def prime(self, source, n):
    assert self.fresh and self.pos == 0
    frames = self.take(n)
    if source == 'truth':
      labels = first_appearance(self.truth[:n])
    else:
      labels = [int(v) for v in oracle.decode(self.model.params, [frames], 1, 1, 1)['labels'][0]]
    labels = np.array(labels, dtype=np.int32)
    start = primed_ref.advance_forced(self.model, frames, labels)
    self.ref = commit_ref.Session(self.model, self.beam, start)
    self.prefix = labels
    self.given.extend(frames)
    return frames, labels, int(_bits(start.score)[0])

  def clusters(self):
    return max([len(h.means) for h in self.ref.beam] or [0])

  def column(self):
    """Every readout of this utterance as a snapshot column (test_gpu_restart._col) plus received and committed."""
    ref, beam = self.ref, self.beam
    inf = _bits(np.full(beam, np.inf)).tolist()
    if ref.received == 0:
      col = {'labels': [], 'scores': 0, 'beam': inf, 'overflow': 0, 'rows': [], 'nb_scores': inf, 'counts': 0, 'stable': 0}
    elif not ref.beam:   # an emptied beam: no hypothesis, labels -1, +inf; what it committed before stays the caller's
      col = {'labels': list(ref.final) + [-1] * ref.have, 'scores': inf[0], 'beam': inf, 'overflow': 0, 'rows': [],
             'nb_scores': inf, 'counts': 0, 'stable': ref.committed}
    else:
      padded = _bits(primed_ref.padded_beam(ref.scores(), beam)).tolist()
      col = {'labels': ref.labels(), 'scores': padded[0], 'beam': padded, 'overflow': 0,
             'rows': [list(ref.final) + r.tolist() for r in ref.rows()], 'nb_scores': padded, 'counts': len(ref.beam),
             'stable': ref.committed + ref.stable()}
    col['received'], col['committed'] = ref.have, ref.committed
    return col


def make_pools(model_name, n_utt, seq_len):
  """POOL_SEQS synthetic sequences per slot, with their speaker ids: (seq float64 [seq_len, D], ids)."""
  dim = int(golden_util.load_case(model_name)['params']['observation_dim'])
  return [[synth.make_utterance(7000 + 100 * u + k, seq_len, dim, mean_segment=4.0) for k in range(POOL_SEQS)] for u in range(n_utt)]


def trace(params, pools, beam, max_frames, plan, max_clusters=16):
  """Run `plan` on the reference.  Returns dict(steps, lives, max_clusters): steps[i] = dict(op, kind, call, result,
  snap, before) -- call: what the device is to be given; result: what it must answer; snap: the column of every slot
  afterwards; before: the columns before (= the previous step's snap).  lives: every _Life, in the order they began."""
  oracle.lib()
  model = primed_ref.Model(params)
  n_utt = len(pools)
  nxt = [0] * n_utt
  lives = []

  def begin(u):
    seq, truth = pools[u][nxt[u] % len(pools[u])]
    nxt[u] += 1
    lives.append(_Life(model, beam, u, seq, truth))
    return lives[-1]

  slots = [begin(u) for u in range(n_utt)]
  log_len = max_frames + 2   # the prior tables: uis_stream_begin's length, lengthened by commits
  steps, most_clusters = [], 0
  snap = [s.column() for s in slots]
  for op in plan:
    before = snap
    kind, call, result = op[0], None, None
    if kind == 'push':
      wants, bad = op[1], op[2] if len(op) > 2 else None
      chunks = []
      for u, s in enumerate(slots):
        room, left = max_frames - s.ref.have, len(s.seq) - s.pos
        n = min(room, left) if wants[u] == 'fill' else min(int(wants[u]), room, left)
        assert not (bad == u and n == 0), 'the non-finite frame was clipped away'
        chunks.append(s.take(n, bad == u) if n else None)
      for s, part in zip(slots, chunks):
        if part is not None:
          s.push(part)
          s.events.append((len(steps), 'push', len(part)))
      call = {'chunks': chunks}
    elif kind == 'commit':
      horizons = None if op[1] is None else [int(v) for v in op[1]]
      have = [s.ref.have for s in slots]
      most = max(s.ref.received for s in slots)
      out = [s.ref.commit(None if horizons is None else horizons[u]) for u, s in enumerate(slots)]
      for s, o in zip(slots, out):
        s.events.append((len(steps), 'commit', o[0]))
      line = None
      if sum(have):   # (a call that finds every window empty does nothing, and says nothing under UIS_COMMIT_TRACE)
        if most + max_frames + 2 > log_len:
          log_len = max(2 * log_len, most + max_frames + 2)
        line = {'window_frames': sum(have), 'committed': sum(len(o[0]) for o in out), 'prior_table_entries': log_len}
      kind = 'commit_none' if horizons is None else 'commit_h'
      call = {'horizons': horizons}
      result = {'labels': [o[0] for o in out], 'dropped': [o[1] for o in out], 'line': line, 'have': have}
    elif kind == 'restart':
      which = [u in op[1] for u in range(n_utt)]
      result = {}
      for u in op[1]:
        col = before[u]
        result[u] = {'labels': col['labels'], 'window': col['labels'][col['committed']:], 'score': col['scores'], 'overflow': 0}
        slots[u].end = (col['labels'], col['scores'])
        slots[u] = begin(u)
      call = {'which': which}
    elif kind == 'prime':
      chunks, labels, result = [None] * n_utt, [None] * n_utt, {}
      for u, (source, n) in sorted(op[1].items()):
        chunks[u], labels[u], result[u] = slots[u].prime(source, max_frames if n == 'window' else int(n))
      call = {'chunks': chunks, 'labels': labels}
    elif kind == 'refuse':
      what, u = op[1], op[2]
      dim = slots[u].seq.shape[1]
      if what == 'push':
        n = max_frames - slots[u].ref.have + int(op[3])
        chunks = [slots[v].seq[slots[v].pos:slots[v].pos + 1] if max_frames > slots[v].ref.have else None for v in range(n_utt)]
        chunks[u] = np.zeros((n, dim))
        call = {'call': 'push', 'chunks': chunks}
      else:
        n = 2 if what == 'prime_received' else max_frames + 1
        assert slots[u].fresh == (what == 'prime_long'), (what, u)
        chunks, labels = [None] * n_utt, [None] * n_utt
        chunks[u], labels[u] = np.tile(slots[u].seq[:1], (n, 1)), np.zeros(n, dtype=np.int32)
        call = {'call': 'prime', 'chunks': chunks, 'labels': labels}
      result = INVALID_ARG
    else:
      raise ValueError(op)
    snap = [s.column() for s in slots]
    most_clusters = max([most_clusters] + [s.clusters() for s in slots])
    steps.append({'op': op, 'kind': kind, 'call': call, 'result': result, 'snap': snap, 'before': before})
  for u, s in enumerate(slots):
    s.end = (snap[u]['labels'], snap[u]['scores'])
  # the cluster cap stays outside the model: no hypothesis of the reference comes near it
  assert most_clusters < max_clusters, (most_clusters, max_clusters)
  return {'steps': steps, 'lives': lives, 'max_clusters': most_clusters, 'n_utt': n_utt, 'beam': beam, 'max_frames': max_frames}


@functools.lru_cache(maxsize=None)
def walk(name):
  """The trace of CASES[name], computed once."""
  case = CASES[name]
  params = golden_util.load_case(case['model'])['params']
  plan = PLANS[case['plan']](case['n_utt'], case['window'], case['seed'])
  pools = make_pools(case['model'], case['n_utt'], case['seq_len'])
  out = trace(params, pools, case['beam'], case['window'], plan, case['cap'])
  out['params'], out['name'] = params, name
  return out


# ---- what a trace reaches

def slot_kinds(tr, u):
  """The operations that touched slot u, in order, as (step, kind): a push that gave it a frame, every commit, a restart
  or a prime that named it."""
  out = []
  for i, st in enumerate(tr['steps']):
    kind = st['kind']
    if kind == 'push' and st['call']['chunks'][u] is not None:
      out.append((i, 'push'))
    elif kind in ('commit_none', 'commit_h'):
      out.append((i, kind))
    elif kind == 'restart' and st['call']['which'][u]:
      out.append((i, 'restart'))
    elif kind == 'prime' and st['call']['chunks'][u] is not None:
      out.append((i, 'prime'))
  return out


def _is(kind, want):
  return kind == want or (want == 'commit' and kind.startswith('commit'))


def facts(tr):
  """The conditions of the walk, each a truth value or a count, from the trace alone."""
  steps, n_utt, beam, window = tr['steps'], tr['n_utt'], tr['beam'], tr['max_frames']
  f = {}
  f['kinds'] = {k: sum(1 for st in steps if st['kind'] == k) for k in KINDS}
  f['bad_frames'] = sum(1 for life in tr['lives'] if life.bad)
  pairs = set()
  for u in range(n_utt):
    seq = slot_kinds(tr, u)
    for (_, a), (_, b) in zip(seq, seq[1:]):
      pairs |= {p for p in PAIRS if _is(a, p[0]) and _is(b, p[1])}
  f['pairs'] = pairs
  # commits
  c = {'dropped': 0, 'overlap': 0, 'no_overlap': 0, 'have_0': 0, 'empty_beam': 0, 'far_horizon': 0}
  for st in steps:
    if not st['kind'].startswith('commit'):
      continue
    res, hz = st['result'], st['call']['horizons']
    for u in range(n_utt):
      have, out, col = res['have'][u], len(res['labels'][u]), st['before'][u]
      c['dropped'] += res['dropped'][u] > 0
      c['overlap'] += out > 0 and have - out > out
      c['no_overlap'] += out > 0 and 0 < have - out <= out
      c['have_0'] += have == 0
      c['empty_beam'] += have > 0 and col['counts'] == 0
      if hz is not None and hz[u] > have > 0 and col['counts'] > 1:
        assert res['dropped'][u] == 0 and out == (col['stable'] - col['committed']) & ~1   # only the stable prefix
        c['far_horizon'] += 1
  f['commits'] = c
  # restarts
  r = {'odd': 0, 'even': 0, 'emptied_window': 0, 'committed': 0, 'empty_beam': 0, 'never': 0}
  per_slot = [0] * n_utt
  for st in steps:
    if st['kind'] != 'restart':
      continue
    for u in st['result']:
      col = st['before'][u]
      per_slot[u] += 1
      r['odd'] += col['received'] % 2 == 1
      r['even'] += col['received'] % 2 == 0 and col['received'] > 0
      r['emptied_window'] += col['received'] == 0 and col['committed'] > 0
      r['committed'] += col['committed'] > 0
      r['empty_beam'] += col['received'] > 0 and col['counts'] == 0
      r['never'] += col['received'] == 0 and col['committed'] == 0
  r['same_slot_twice'] = max(per_slot) >= 2
  f['restarts'] = r
  # primes
  p = {'restarted_between_odd_and_even': 0, 'whole_window_then_room': 0}
  for i, st in enumerate(steps):
    if st['kind'] != 'prime':
      continue
    for u in st['result']:
      just = _last_kind(tr, u, i) == 'restart'
      parity = {st['before'][v]['received'] % 2 for v in range(n_utt) if v != u and st['before'][v]['received'] > 0}
      p['restarted_between_odd_and_even'] += just and parity == {0, 1}
      if len(st['call']['labels'][u]) == window:
        nxt = [s for s in steps[i + 1:] if s['kind'].startswith('commit')]
        p['whole_window_then_room'] += bool(nxt) and len(nxt[0]['result']['labels'][u]) > 0
  f['primes'] = p
  # long lives: more frames than the prior tables were opened for
  longest = max(len(life.given) for life in tr['lives'])
  per_slot_frames = [{} for _ in range(n_utt)]
  for life in tr['lives']:
    per_slot_frames[life.slot][id(life)] = len(life.given)
  f['one_life_outgrows_the_tables'] = longest > 2 * window + 2
  f['a_slot_outgrows_the_tables_across_a_restart'] = any(   # (another slot than the one with the longest life)
      len(d) >= 2 and sum(d.values()) > 2 * window + 2 and max(d.values()) < longest for d in per_slot_frames)
  f['tables_grew'] = max([st['result']['line']['prior_table_entries'] for st in steps
                          if st['kind'].startswith('commit') and st['result']['line']] or [0]) > window + 2
  # a beam narrowed by a prune that fills up again (the same utterance: no restart in between)
  narrow = False
  for u in range(n_utt):
    state = 0
    for st in steps:
      if st['kind'] == 'restart' and st['call']['which'][u]:
        state = 0
      elif st['kind'] == 'commit_h' and st['result']['dropped'][u] > 0 and 0 < st['snap'][u]['counts'] < beam:
        state = 1
      elif state == 1 and st['snap'][u]['counts'] == beam:
        narrow = True
  f['a_pruned_beam_fills_up_again'] = narrow
  # refusals, each in a session that is not trivial: some slot has committed, some beam holds several hypotheses
  ref = {}
  for st in steps:
    if st['kind'] == 'refuse':
      busy = any(c['committed'] > 0 for c in st['before']) and any(c['counts'] > 1 for c in st['before'])
      ref[st['op'][1]] = ref.get(st['op'][1], 0) + (1 if busy else 0)
      assert st['snap'] == st['before']
  f['refusals'] = ref
  f['a_push_fills_a_window'] = any(st['kind'] == 'push' and st['call']['chunks'][u] is not None and
                                   st['snap'][u]['received'] == window and st['snap'][u]['counts'] > 1
                                   for st in steps for u in range(n_utt))
  f['frames'] = sum(len(life.given) for life in tr['lives'])
  f['operations'] = len(steps)
  return f


def _last_kind(tr, u, i):
  """The kind of the last operation before step i that touched slot u (commits aside: they touch every slot)."""
  last = None
  for j, k in slot_kinds(tr, u):
    if j >= i:
      break
    if not k.startswith('commit'):
      last = k
  return last
