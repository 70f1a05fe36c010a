"""The cases of the tagged-session tests: shapes, plans and their traces on the CPU reference.  No device, no library.

Shapes are tests/session_walk.py's (model, slots, beam, window, cap).  A PLAN is a list of operations written without
knowing what the model answers; trace() runs it on tests/known_session_ref.py's Session, one object per slot, and
returns for every operation the call as the device is to receive it, the result it must give, and the snapshot of
every slot afterwards -- the n-best rows, the scores' bits, uis_stream_bindings' row, the frame counts.  Every trace is
computed once (functools.lru_cache) and shared; nobody writes into it.

  ('push', counts[, what])   counts[u] frames for slot u (0: silent).  what: a set of 'tags' (known_ref.pattern of the
                             slot's life), 'zeros' (an all-zero table), 'bias' (soft_bias)
  ('tag', {slot: tag})       one frame for each slot named, carrying that tag
  ('commit', horizons)       None, or one int per slot (negative: none)
  ('query',)                 uis_stream_retire as a query
  ('retire', {slot: [k]})    a list per slot, present indices
  ('restart', slots)         the slots end; each goes on with its next sequence (and that life's tag pattern)
  ('prime', {slot: n})       n frames, labels = the first-appearance form of the sequence's speaker ids, under the tags
                             that those labels force (tag = 1 + label at every other frame)
  ('prime', {slot: (labels, tags)})   the same with both given
"""

import functools
import types

import numpy as np

import golden_util
import known_ref
import known_session_ref
import primed_ref
import session_walk as sw
from oracle import oracle
from uisrnn_amd import synth

SHAPES = ('small4', 'small10', 'deep', 'one_launch')
RESIDENT_SHAPES = ('one_launch',)   # where uis_stream_begin accepts UIS_FLAG_RESIDENT (depth 1, D and H of a one-launch kernel)
CHUNKINGS = ('one', 'three', 'ragged', 'whole')
LIVES = 3         # sequences per slot: a restart takes the next one
SEQ_LEN = 40


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def shape(name):
  case = sw.CASES[name]
  oracle.lib()
  params = golden_util.load_case(case['model'])['params']
  dim = int(params['observation_dim'])
  pool = [[synth.make_utterance(7000 + 100 * u + k, SEQ_LEN, dim, mean_segment=4.0) for k in range(LIVES)]
          for u in range(case['n_utt'])]
  return types.SimpleNamespace(name=name, params=params, model=primed_ref.Model(params), n_utt=case['n_utt'],
                               beam=case['beam'], window=case['window'], cap=case['cap'], pool=pool)


def life_tags(u, life, n):
  return known_ref.pattern(u + life, n)


def soft_bias(u, n):
  """NaN (the model's), 0.3, 0.7 in turn: no hard constraint, so no beam empties."""
  return np.array([(np.nan, 0.3, 0.7)[(t + u) % 3] for t in range(n)], dtype=np.float64)


def chunk_lengths(sh):
  return [sh.window - u % 3 for u in range(sh.n_utt)]


def schedule(kind, lengths):
  """Per push the frames of every slot.  ragged: push r gives slot u (r + u) % 4 frames -- 0: the slot is silent."""
  left, out, r = list(lengths), [], 0
  while any(left):
    want = {'one': lambda u: 1, 'three': lambda u: 3, 'ragged': lambda u: (r + u) % 4, 'whole': lambda u: left[u]}[kind]
    counts = [min(want(u), left[u]) for u in range(len(left))]
    r += 1
    if not any(counts):
      continue
    left = [a - b for a, b in zip(left, counts)]
    out.append(tuple(counts))
  return out


def chunk_calls(sh, kind):
  """The pushes of a chunking as the device is to receive them, (chunks, speakers), without running the reference."""
  lengths = chunk_lengths(sh)
  pos, out = [0] * sh.n_utt, []
  for counts in schedule(kind, lengths):
    chunks = [sh.pool[u][0][0][pos[u]:pos[u] + c] if c else None for u, c in enumerate(counts)]
    flat = np.concatenate([life_tags(u, 0, SEQ_LEN)[pos[u]:pos[u] + c] for u, c in enumerate(counts)])
    pos = [p + c for p, c in zip(pos, counts)]
    out.append((chunks, flat))
  return out


def chunk_plan(sh, kind, what=('tags',)):
  return tuple(('push', counts, frozenset(what)) for counts in schedule(kind, chunk_lengths(sh)))


def snap(sessions):
  out = []
  for s in sessions:
    rows = s.rows()
    out.append({'rows': rows.tolist(), 'scores': _bits(s.scores()).tolist(), 'bind': s.bindings_row().tolist(),
                'have': s.have, 'committed': s.committed, 'live': s.live, 'K': s.K(),
                'tagged': s.tagged(), 'retirable': s.retirable()})
  return out


def _trace(sh, plan, limits=None):
  n_utt = sh.n_utt
  life = [0] * n_utt
  pos = [0] * n_utt

  def fresh(u):
    return known_session_ref.Session(sh.model, sh.beam, limit=None if limits is None else limits[u])

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
        if 'zeros' in what:
          g = np.zeros_like(g)
        chunks[u] = part
        sessions[u].push(part, g if what & {'tags', 'zeros'} else None, b if 'bias' in what else None)
        tags.append(g)
        bias.append(b)
      call = {'chunks': chunks,
              'speakers': np.concatenate(tags) if tags and what & {'tags', 'zeros'} else None,
              'bias': np.concatenate(bias) if bias and 'bias' in what else None}
    elif kind == 'commit':
      horizons = None if op[1] is None else [int(v) for v in op[1]]
      out = [s.commit(None if horizons is None or horizons[u] < 0 else horizons[u]) for u, s in enumerate(sessions)]
      call = {'horizons': horizons}
      # (the library hands out present indices; retire_ref's commit returns stream ids)
      result = {'labels': [[known_session_ref.retire_ref.to_local(c, s.gone) for c in o[0]] for o, s in zip(out, sessions)],
                'dropped': [o[1] for o in out]}
    elif kind == 'query':
      result = {'retirable': [s.retirable() for s in sessions], 'tagged': [s.tagged() for s in sessions]}
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
      chunks, labels, tags, result = [None] * n_utt, [None] * n_utt, [], {}
      for u, n in sorted(op[1].items()):
        assert sessions[u].received == 0
        if isinstance(n, tuple):
          lab, g = np.array(n[0], dtype=np.int32), np.array(n[1], dtype=np.uint8)
        else:
          lab = np.array(sw.first_appearance(sh.pool[u][life[u]][1][:n]), dtype=np.int32)
          g = np.array([1 + c if t % 2 == 0 else 0 for t, c in enumerate(lab)], dtype=np.uint8)
        part, _, _ = take(u, len(lab))
        start = known_session_ref.primed(sh.model, part, lab, g)
        sessions[u] = known_session_ref.Session(sh.model, sh.beam, start, None if limits is None else limits[u])
        chunks[u], labels[u] = part, lab
        tags.append(g)
        result[u] = int(_bits(start.score)[0])
      call = {'chunks': chunks, 'labels': labels, 'speakers': np.concatenate(tags)}
    else:
      raise ValueError(op)
    steps.append({'op': op, 'kind': kind, 'call': call, 'result': result, 'snap': snap(sessions)})
  return steps


@functools.lru_cache(maxsize=None)
def untagged_rows(name):
  """The best labels of the chunk case's frames without tags: what the tags must change."""
  sh = shape(name)
  out = []
  for u, n in enumerate(chunk_lengths(sh)):
    s = known_session_ref.Session(sh.model, sh.beam)
    s.push(sh.pool[u][0][0][:n])
    out.append(s.rows()[0].tolist())
  return out


# ---- the plans

T = frozenset(('tags',))


def everyone(sh, n):
  return tuple([n] * sh.n_utt)


def commit_plan(sh):
  """Tagged pushes with a commit of the stable prefix and commits with horizons between them, past the window's length."""
  return (('push', everyone(sh, sh.window - 3), T), ('commit', None), ('push', everyone(sh, 2), T),
          ('commit', tuple(3 + u % 2 for u in range(sh.n_utt))), ('push', everyone(sh, 5), T), ('commit', tuple([0] * sh.n_utt)),
          ('push', everyone(sh, 3), T))


RETIRE_PREFIX = ((0, 0, 1, 1, 2, 2), (0, 0, 5, 5, 0, 0))   # slot 0: cluster 0 without a tag, cluster 1 under tag 5, last label 2


def retire_plan(sh):
  """Slot 0 is primed with RETIRE_PREFIX and a commit with horizon 0 empties its window: clusters 0 and 1 lie before the
  window and neither is the last label, so both would be retirable -- but cluster 1 carries tag 5.  The query must list
  cluster 0 alone; retiring it moves the binding of tag 5 from index 1 to index 0; the frames tagged 5 that follow must
  land there.  The other slots decode under the pattern meanwhile."""
  counts = tuple([0] + [4] * (sh.n_utt - 1))
  return (('prime', {0: RETIRE_PREFIX}), ('push', counts, T), ('commit', tuple([0] + [-1] * (sh.n_utt - 1))), ('query',),
          ('retire', {0: [0]}), ('query',), ('tag', {0: 5}), ('tag', {0: 5}), ('push', everyone(sh, 3), T), ('query',))


def restart_plan(sh):
  """Slot 1 ends after five tagged frames; its next utterance meets tag 1 again and binds it afresh."""
  return (('push', everyone(sh, 5), T), ('restart', (1,)), ('tag', {1: 1}), ('push', everyone(sh, 4), T), ('push', everyone(sh, 2), T))


PRIME_PREFIXES = {0: ((0, 0, 1, 1, 0, 2), (1, 0, 0, 2, 1, 0)),   # tags 1 and 2 of the pattern bound ahead of it, cluster 2 free
                  2: ((0, 1, 1, 0, 1), (0, 3, 0, 0, 3))}        # tag 3 on the second cluster


def prime_plan(sh):
  return (('prime', dict(PRIME_PREFIXES)), ('push', everyone(sh, 4), T), ('push', everyone(sh, 2), T))


def tag127_plan(sh):
  """Tag 127 at every slot's first frame, then the pattern."""
  return (('tag', {u: 127 for u in range(sh.n_utt)}), ('push', everyone(sh, 5), T))


def all_bound_plan(sh):
  """Four frames under four different tags: every cluster of every hypothesis is bound.  Then a fifth tag (only the new
  cluster may take it), tag 2 again (only its cluster may), and two frames without a table."""
  every = lambda g: {u: g for u in range(sh.n_utt)}   # pylint: disable=unnecessary-lambda-assignment
  return tuple(('tag', every(g)) for g in (1, 2, 3, 4, 5, 2)) + (('push', everyone(sh, 2)),)


def together_plan(sh):
  """Tags, a bias table and max_speakers (TOGETHER_LIMITS) in force in the same pushes."""
  both = frozenset(('tags', 'bias'))
  return (('push', everyone(sh, 3), both), ('push', tuple(u % 3 for u in range(sh.n_utt)), both), ('push', everyone(sh, 6), both))


def together_limits(sh):
  return tuple(3 + u % 2 for u in range(sh.n_utt))   # (the pattern names three speakers: each has room)


PLANS = {'commit': commit_plan, 'retire': retire_plan, 'restart': restart_plan, 'prime': prime_plan, 'tag127': tag127_plan,
         'all_bound': all_bound_plan, 'together': together_plan}
PLANS.update({'chunk_' + kind: functools.partial(lambda sh, kind: chunk_plan(sh, kind), kind=kind) for kind in CHUNKINGS})
PLANS['zeros'] = lambda sh: chunk_plan(sh, 'three', ('zeros',))
PLANS['plain'] = lambda sh: chunk_plan(sh, 'three', ())


@functools.lru_cache(maxsize=None)
def trace(name, plan):
  """The trace of PLANS[plan] on shape `name`, computed once."""
  sh = shape(name)
  return _trace(sh, PLANS[plan](sh), together_limits(sh) if plan == 'together' else None)
