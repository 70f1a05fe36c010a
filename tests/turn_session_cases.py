"""The cases of the minimum-turn-length session tests: shapes, plans and their traces on the CPU reference.  No device, no
library.

Shapes are tests/session_walk.py's (model, slots, beam, window, cap), as tests/known_session_cases.py reads them, with a
pool of sequences of this module's own: SEEDS names, per shape, the first seed of 0 .. 8 under which m = 3 on every slot
changes the labels of some slot of the chunk case, empties no beam and keeps every K under the cap, and under which the
per-slot values change a slot's labels too (found on the CPU; tests/test_turn_session_host.py asserts both).  A slot's value is M_VALUES[u % 4], so ruled and unruled slots share every
launch.  A PLAN is a list of operations written without knowing what the model answers; trace() runs it on
tests/turn_session_ref.py's Session, one object per slot, and returns for every operation the call as the device is to
receive it, the result it must give, and the snapshot of every slot afterwards -- the n-best rows, the scores' bits,
uis_session_turns' row, every live rank's (label, run), the frame counts.  Every trace is computed once and shared;
nobody writes into it.

  ('push', counts[, what])   counts[u] frames for slot u (0: silent); what: a set of 'tags' (known_ref.pattern), 'onetag'
                             (the pattern's tagged frames, all under the slot's one tag 1 + u % 3), 'bias'
  ('tag', {slot: tag})       one frame for each slot named, carrying that tag
  ('commit', horizons)       None, or one int per slot (negative: none)
  ('query',)                 uis_stream_retire as a query
  ('retire', {slot: [k]})    a list per slot, present indices
  ('restart', slots)         the slots end; each goes on with its next sequence
  ('prime', {slot: labels})  len(labels) frames under the given labels
  ('setm', values)           uis_session_min_turn: one value per slot (the plan keeps to the fresh-slot rule)
"""

import functools
import types

import numpy as np

import golden_util
import known_session_cases as kc
import known_session_ref
import primed_ref
import session_walk as sw
import turn_session_ref as tsr
from oracle import oracle
from uisrnn_amd import synth

SHAPES = kc.SHAPES
RESIDENT_SHAPES = kc.RESIDENT_SHAPES
CHUNKINGS = kc.CHUNKINGS
LIVES = 3
SEQ_LEN = kc.SEQ_LEN
M = 3
M_VALUES = (0, 2, 3, 5)
SEEDS = {'small4': 6, 'small10': 7, 'deep': 2, 'one_launch': 0}


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def slot_values(n_utt):
  return [M_VALUES[u % 4] for u in range(n_utt)]


@functools.lru_cache(maxsize=None)
def shape(name, seed=None):
  case = sw.CASES[name]
  oracle.lib()
  params = golden_util.load_case(case['model'])['params']
  dim = int(params['observation_dim'])
  seed = SEEDS[name] if seed is None else seed
  # (short segments: the model changes speaker after one or two frames often enough for the rule to have work)
  pool = [[synth.make_utterance(9000 + 1000 * seed + 100 * u + k, SEQ_LEN, dim, mean_segment=2.0) for k in range(LIVES)]
          for u in range(case['n_utt'])]
  return types.SimpleNamespace(name=name, params=params, model=primed_ref.Model(params), n_utt=case['n_utt'],
                               beam=case['beam'], window=case['window'], cap=case['cap'], pool=pool)


chunk_lengths = kc.chunk_lengths
schedule = kc.schedule
life_tags = kc.life_tags
soft_bias = kc.soft_bias


def chunk_calls(sh, kind):
  """The pushes of a chunking as the device is to receive them, without running the reference."""
  lengths = chunk_lengths(sh)
  pos, out = [0] * sh.n_utt, []
  for counts in schedule(kind, lengths):
    out.append([sh.pool[u][0][0][pos[u]:pos[u] + c] if c else None for u, c in enumerate(counts)])
    pos = [p + c for p, c in zip(pos, counts)]
  return out


def chunk_plan(sh, kind, values=None):
  values = slot_values(sh.n_utt) if values is None else list(values)
  return (('setm', tuple(values)),) + tuple(('push', counts) for counts in schedule(kind, chunk_lengths(sh)))


def snap(sessions):
  out = []
  for s in sessions:
    out.append({'rows': s.rows().tolist(), 'scores': _bits(s.scores()).tolist(), 'turns': s.turns_row(),
                'words': [list(w) for w in s.exported()], 'have': s.have, 'committed': s.committed, 'live': s.live,
                'K': s.K(), 'retirable': s.retirable(), 'm': s.m})
  return out


def _trace(sh, plan, limits=None):
  n_utt = sh.n_utt
  life, pos, values = [0] * n_utt, [0] * n_utt, [0] * n_utt

  def fresh(u, start=None):
    return tsr.Session(sh.model, sh.beam, start, None if limits is None else limits[u], values[u])

  sessions = [fresh(u) for u in range(n_utt)]
  steps = []

  def take(u, n):
    seq = sh.pool[u][life[u]][0]
    assert pos[u] + n <= len(seq), 'the plan outruns its sequences'
    assert sessions[u].have + n <= sh.window, 'the plan outruns the session\'s window'
    part = seq[pos[u]:pos[u] + n]
    tags = life_tags(u, life[u], len(seq))[pos[u]:pos[u] + n]
    bias = soft_bias(u, len(seq))[pos[u]:pos[u] + n]
    pos[u] += n
    return part, tags, bias

  for op in plan:
    kind, call, result = op[0], None, None
    if kind in ('push', 'tag'):
      if kind == 'tag':
        counts, what = [1 if u in op[1] else 0 for u in range(n_utt)], frozenset(('tags',))
      else:
        counts, what = op[1], op[2] if len(op) > 2 else frozenset()
      chunks, tags, bias = [None] * n_utt, [], []
      for u in range(n_utt):
        if not counts[u]:
          continue
        part, g, b = take(u, counts[u])
        if kind == 'tag':
          g = np.full(1, op[1][u], dtype=np.uint8)
        if 'onetag' in what:   # (one known speaker per slot: the pattern's tagged frames, all under the slot's own tag)
          g = np.where(g > 0, 1 + u % 3, 0).astype(np.uint8)
        chunks[u] = part
        sessions[u].push(part, g if what & {'tags', 'onetag'} else None, b if 'bias' in what else None)
        tags.append(g)
        bias.append(b)
      call = {'chunks': chunks, 'speakers': np.concatenate(tags) if tags and what & {'tags', 'onetag'} else None,
              'bias': np.concatenate(bias) if bias and 'bias' in what else None}
    elif kind == 'commit':
      horizons = None if op[1] is None else [int(v) for v in op[1]]
      out = [s.commit(None if horizons is None or horizons[u] < 0 else horizons[u]) for u, s in enumerate(sessions)]
      call = {'horizons': horizons}
      result = {'labels': [[known_session_ref.retire_ref.to_local(c, s.gone) for c in o[0]] for o, s in zip(out, sessions)],
                'dropped': [o[1] for o in out]}
    elif kind == 'query':
      result = {'retirable': [s.retirable() for s in sessions]}
    elif kind == 'retire':
      call = {'clusters': [sorted(op[1].get(u, [])) or None for u in range(n_utt)]}
      for u, ks in op[1].items():
        sessions[u].retire(ks)
    elif kind == 'restart':
      for u in op[1]:
        life[u] += 1
        pos[u] = 0
        sessions[u] = fresh(u)
      call = {'which': [u in op[1] for u in range(n_utt)]}
    elif kind == 'prime':
      chunks, labels, result = [None] * n_utt, [None] * n_utt, {}
      for u, lab in sorted(op[1].items()):
        assert sessions[u].received == 0
        lab = np.array(lab, dtype=np.int32)
        part, _, _ = take(u, len(lab))
        start = tsr.primed(sh.model, part, lab)
        sessions[u] = fresh(u, start)
        chunks[u], labels[u] = part, lab
        result[u] = int(_bits(start.score)[0])
      call = {'chunks': chunks, 'labels': labels}
    elif kind == 'setm':
      new = [int(v) for v in op[1]]
      for u in range(n_utt):
        assert new[u] == values[u] or sessions[u].received == 0, 'the plan breaks the fresh-slot rule'
        values[u] = new[u]
        sessions[u].m = new[u]
      call = {'values': new}
    else:
      raise ValueError(op)
    steps.append({'op': op, 'kind': kind, 'call': call, 'result': result, 'snap': snap(sessions)})
  return steps


# ---- the plans

def everyone(sh, n):
  return tuple([n] * sh.n_utt)


def values_of(sh):
  return tuple(slot_values(sh.n_utt))


def commit_plan(sh):
  """Pushes with a commit of the stable prefix and commits with horizons between them, one of which (horizon 0) empties
  every window; the pushes that follow go on from the runs the commits moved."""
  return (('setm', values_of(sh)), ('push', everyone(sh, sh.window - 3)), ('commit', None), ('push', everyone(sh, 2)),
          ('commit', tuple(3 + u % 2 for u in range(sh.n_utt))), ('push', everyone(sh, 5)), ('commit', tuple([0] * sh.n_utt)),
          ('push', everyone(sh, 1)), ('push', everyone(sh, 3)))


RETIRE_PREFIX = (0, 0, 0, 1, 1, 1, 2, 2)   # slot 0 under m = 3: the hypothesis is in cluster 2, two frames into its turn


def retire_plan(sh):
  """Slot 0 is primed with RETIRE_PREFIX under m = 3 and a commit with horizon 0 empties its window: clusters 0 and 1 lie
  before the window, the hypothesis speaks in cluster 2 with run 2.  The query lists 0 and 1 and not 2; retiring both
  leaves label 0 with run 2, and the next push holds the hypothesis for one more frame."""
  counts = tuple([0] + [4] * (sh.n_utt - 1))
  values = tuple([M] + list(values_of(sh))[1:])
  return (('setm', values), ('prime', {0: RETIRE_PREFIX}), ('push', counts), ('commit', tuple([0] + [-1] * (sh.n_utt - 1))),
          ('query',), ('retire', {0: [0, 1]}), ('query',), ('push', everyone(sh, 1)), ('push', everyone(sh, 1)),
          ('push', everyone(sh, 3)), ('query',))


PRIME_PREFIXES = {0: (0, 0, 1, 0, 0), 1: (0, 1, 1), 2: (0, 0, 0, 0, 1)}   # a one-frame turn inside; runs 2, 2 and 1


def prime_plan(sh):
  """Slots 0 .. 2 are primed under m = 3, 2 and 3 (slot 0's value is set for the purpose)."""
  values = tuple([M] + list(values_of(sh))[1:])
  return (('setm', values), ('prime', dict(PRIME_PREFIXES)), ('push', everyone(sh, 1)), ('push', everyone(sh, 4)),
          ('push', everyone(sh, 2)))


def restart_plan(sh):
  """Slot 2 (m = 3) ends after four frames; its next utterance starts without a run under the same value; after the
  restart its value changes to 5."""
  v = list(values_of(sh))
  w = list(v)
  w[2] = 5
  return (('setm', tuple(v)), ('push', everyone(sh, 4)), ('restart', (2,)), ('push', everyone(sh, 3)), ('restart', (2,)),
          ('setm', tuple(w)), ('push', everyone(sh, 4)))


def together_plan(sh):
  """The rule, tags, a soft bias table and max_speakers (together_limits) in the same pushes.  Every slot hears one
  known speaker (two different tags closer than m frames contradict the rule: that is slot 2's part).  Slot 2 (m = 3)
  meets two different tags on its first two frames: its beam empties, and it is compared all the same."""
  both = frozenset(('onetag', 'bias'))
  return (('setm', values_of(sh)), ('tag', {2: 1}), ('tag', {2: 2}), ('push', everyone(sh, 3), both),
          ('push', tuple(u % 3 for u in range(sh.n_utt)), both), ('push', everyone(sh, 5), both))


def together_limits(sh):
  return tuple([3] * sh.n_utt)


PLANS = {'commit': commit_plan, 'retire': retire_plan, 'prime': prime_plan, 'restart': restart_plan,
         'together': together_plan}
PLANS.update({'chunk_' + kind: functools.partial(lambda sh, kind: chunk_plan(sh, kind), kind=kind) for kind in CHUNKINGS})
PLANS['zeros_ones'] = lambda sh: chunk_plan(sh, 'three', [u % 2 for u in range(sh.n_utt)])
PLANS['plain'] = lambda sh: chunk_plan(sh, 'three', [0] * sh.n_utt)[1:]
PLANS['all3'] = lambda sh: chunk_plan(sh, 'whole', [M] * sh.n_utt)
PLANS['free'] = lambda sh: chunk_plan(sh, 'whole', [0] * sh.n_utt)


@functools.lru_cache(maxsize=None)
def trace(name, plan, seed=None):
  """The trace of PLANS[plan] on shape `name`, computed once."""
  sh = shape(name, seed)
  return _trace(sh, PLANS[plan](sh), together_limits(sh) if plan == 'together' else None)


def bites(name, seed=None):
  """Whether m = 3 on every slot of the chunk case changes some slot's labels, empties no beam and keeps every K under
  the cap: (changed slots, emptied slots, largest K)."""
  sh = shape(name, seed)
  free, ruled = trace(name, 'free', seed)[-1]['snap'], trace(name, 'all3', seed)[-1]['snap']
  changed = [u for u in range(sh.n_utt) if ruled[u]['live'] and ruled[u]['rows'][0] != free[u]['rows'][0]]
  emptied = [u for u in range(sh.n_utt) if not ruled[u]['live']]
  return changed, emptied, max(col['K'] for col in ruled)
