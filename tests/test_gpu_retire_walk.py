"""A random walk over a session that retires clusters, against tests/retire_ref.py after every operation.

200 operations per seed over {push, commit with and without horizons, query, retire everything retirable, retire a
random valid subset, restart} on a two-slot session whose streams walk through many speakers under a cluster cap of
8.  The operations are drawn in lock-step with the reference (a valid subset needs the reference's retirable set) and
the reference alone steers the walk away from the cap and the end of the window: a slot that could pass either with
three more frames commits and retires first and, where that does not help, restarts.  Every readout of
tests/test_gpu_retire.py's snapshot is compared after every operation, exactly.
"""

import numpy as np
import pytest

import retire_ref
import test_gpu_retire as tr
from session_walk import POOL_SEQS

pytestmark = pytest.mark.gpu

N_UTT, BEAM, CAP, WINDOW, OPS = 2, 3, 8, 16, 200


def _pool(seed, u):
  return [retire_ref.speaker_walk(9000 + 100 * seed + 10 * u + k, 64, 7, 2, 400) for k in range(POOL_SEQS)]


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_a_random_walk_with_retirements(seed, oracle_lib):
  rng = np.random.default_rng(seed)
  model = tr._model()   # pylint: disable=protected-access
  pools = [_pool(seed, u) for u in range(N_UTT)]
  life = [0] * N_UTT      # which sequence of its pool a slot is on
  pos = [0] * N_UTT
  refs = [retire_ref.Session(model, BEAM) for _ in range(N_UTT)]
  done = {k: 0 for k in ('push', 'commit', 'commit_h', 'query', 'retire_all', 'retire_subset', 'restart', 'retired', 'forced')}
  dev = tr.Dev(N_UTT, BEAM, WINDOW, CAP)

  def most(ref):
    return max([len(h.means) for h in ref.beam] or [0])

  def restart(which, what):
    want = {u: refs[u].labels() for u in which}
    assert dev.restart(which) == want, what
    for u in which:
      refs[u] = retire_ref.Session(model, BEAM)
      life[u] += 1
      pos[u] = 0
    done['restart'] += 1
    tr.same(dev, refs, what)

  try:
    n_ops = 0
    while n_ops < OPS:
      what = (seed, n_ops)
      n_ops += 1
      r = rng.random()
      tight = [u for u in range(N_UTT) if most(refs[u]) + 3 > CAP or refs[u].have + 3 > WINDOW]
      if r < 0.45 and tight:      # the reference steers: make room first (these count as operations of the walk)
        tr.both_commit(dev, refs, [2 if u in tight else -1 for u in range(N_UTT)], what)
        tr.both_retire(dev, refs, tight, what)
        n_ops += 1
        done['forced'] += 1
        done['retired'] += sum(len(ref.retired[-1]) for ref in refs)
        still = [u for u in tight if most(refs[u]) + 3 > CAP or refs[u].have + 3 > WINDOW]
        if still:
          restart(still, what)
          n_ops += 1
      elif r < 0.45:
        sizes = [int(rng.integers(0, 4)) for _ in range(N_UTT)]
        chunks = []
        for u in range(N_UTT):
          seq = pools[u][life[u] % POOL_SEQS]
          chunks.append(seq[pos[u]:pos[u] + sizes[u]] if sizes[u] else None)
          pos[u] += sizes[u]
        tr.both_push(dev, refs, chunks, CAP, what)
        done['push'] += 1
      elif r < 0.52:
        tr.both_commit(dev, refs, [-1] * N_UTT, what)
        done['commit'] += 1
      elif r < 0.62:
        tr.both_commit(dev, refs, [int(rng.choice([-1, 0, 2, 3, 5])) for _ in range(N_UTT)], what)
        done['commit_h'] += 1
      elif r < 0.70:
        before = tr.plain(tr.same(dev, refs, what))
        res = dev.dec.stream_retire(clusters=[None] * N_UTT)
        assert res['K'].tolist() == [ref.K() for ref in refs] and tr.plain(dev.shot()) == before, what
        done['query'] += 1
      elif r < 0.82:
        which = [None, [0], [1]][int(rng.integers(0, 3))]
        tr.both_retire(dev, refs, which, what)
        done['retire_all'] += 1
        done['retired'] += sum(len(ref.retired[-1]) for ref in refs)
      elif r < 0.94:
        picks = []
        for ref in refs:
          able = ref.retirable()
          picks.append([k for k in able if rng.random() < 0.5] or None)
        tr.both_retire(dev, refs, None, what, clusters=picks)
        done['retire_subset'] += 1
        done['retired'] += sum(len(ref.retired[-1]) for ref in refs)
      else:
        restart([int(rng.integers(0, N_UTT))], what)
  finally:
    dev.close()
  # the walk went where it is meant to go
  assert all(done[k] > 0 for k in done), done
  assert done['retired'] >= 10, done
