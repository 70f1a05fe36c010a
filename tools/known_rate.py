"""What known speakers cost on the MI355X.  Nothing here is a threshold: the figures are
recorded, losses included.

  python tools/known_rate.py untagged --parent DIR [--runs 5] [--configs 2,4] [--out profiles/known_rate.json]
  python tools/known_rate.py cost     [--frames 500] [--steps 3]

trained_d256, synthetic utterances (uisrnn_amd.synth), 64 utterances.
  untagged  what the decode without a table pays for the feature: bench.py --gpus 1 at configs 2 and 4 (whose kernels the
            rule touches) and 1 and 3 (which it must not), this tree and a built checkout of the parent commit (--parent)
            interleaved in one session, --runs each; the two ranges of frames/s and whether they overlap.
  cost      64 x --frames, beam 10, test_iteration 2 (configs[1]'s shape): the decode under a table (k_decode_resident)
            against the decode without one (k_decode_rs: the planner exclusion), and against the decode without one
            under UIS_FLAG_OWNER_SELECT (the same kernel: the rule plus the table's upload).  Device milliseconds and
            wall time per call.
The table: a corrected transcript's shape -- every third frame carries the name of its true speaker.  Every leg merges
its keys into --out.
"""

import argparse
import json
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, 'tools'))

import bias_rate  # noqa: E402  pylint: disable=wrong-import-position
import score_rate  # noqa: E402  pylint: disable=wrong-import-position
from uisrnn_amd import _capi, synth, weights  # noqa: E402  pylint: disable=wrong-import-position


def _tags(truth, u=0):
  """Every third frame's true speaker, as tags 1 .. 127 in the order they first appear."""
  seen = {}
  tags = np.zeros(len(truth), dtype=np.uint8)
  for t, name in enumerate(truth):
    if (t + u) % 3 == 0:
      tags[t] = seen.setdefault(name, len(seen) + 1)
  return tags


def _timed_decode(dec, seqs, steps, warmup, flags=0, speakers=None):
  import time  # pylint: disable=import-outside-toplevel
  wall, dev = [], []
  for k in range(warmup + steps):
    t0 = time.perf_counter()
    out = dec.decode_f64(seqs, 10, 1, 2, flags=flags, speakers=speakers)
    if k >= warmup:
      wall.append(time.perf_counter() - t0)
      dev.append(out['stats']['decode_ms'])
  frames = sum(s.shape[0] for s in seqs)
  return {'ms_per_call': 1e3 * float(np.median(wall)), 'device_ms': float(np.median(dev)),
          'frames_per_s_device': frames / (float(np.median(dev)) / 1e3), 'decode_kernel': out['stats']['decode_kernel'],
          'instantiation': list(dec.last_instantiation()), 'overflow': int(out['overflow'].any()),
          'speakers_found': int(max(out['labels'].max(), -1)) + 1}


def leg_cost(params, a):
  pairs = [synth.make_utterance(7000 + u, a.frames, int(params['observation_dim'])) for u in range(a.utterances)]
  seqs = [p[0] for p in pairs]
  speakers = np.concatenate([_tags(list(p[1]), u) for u, p in enumerate(pairs)])
  dec = _capi.Decoder(params)
  try:
    res = {'utterances': a.utterances, 'frames': a.frames, 'beam': 10, 'test_iteration': 2,
           'tagged_share': float((speakers != 0).mean()),
           'no_table': _timed_decode(dec, seqs, a.steps, a.warmup),
           'no_table_owner_select': _timed_decode(dec, seqs, a.steps, a.warmup, flags=_capi.UIS_FLAG_OWNER_SELECT),
           'table': _timed_decode(dec, seqs, a.steps, a.warmup, speakers=speakers)}
  finally:
    dec.close()
  return res


def leg_untagged(a):
  if not a.parent or not os.path.exists(os.path.join(a.parent, 'bench.py')):
    raise SystemExit('--parent: a checkout of the parent commit with its library built')
  how = ('bench.py --gpus 1 --warmup 2 --no_cpu_baseline --no_extra_configs --no_host_buffers; the parent commit and '
         'this one interleaved in one session')
  res = {}   # (one key per config: a later session of the same config replaces it, whatever else it measured)
  for config, steps in ((2, 3), (4, 3), (1, 10), (3, 3)):
    if config not in a.configs:
      continue
    rows = {'parent': [], 'this_commit': []}
    for _ in range(a.runs):
      rows['parent'].append(bias_rate._bench(a.parent, config, steps))  # pylint: disable=protected-access
      rows['this_commit'].append(bias_rate._bench(_ROOT, config, steps))  # pylint: disable=protected-access
      print(config, rows['parent'][-1], rows['this_commit'][-1], flush=True)
    lo, hi = min(rows['this_commit']), max(rows['this_commit'])
    overlap = hi >= min(rows['parent']) and lo <= max(rows['parent'])
    res['untagged_against_the_parent_commit_config_%d' % config] = {
        'how': how, 'runs_each': a.runs, 'steps': steps, 'frames_per_s': rows,
        'verdict': 'one pair of runs: no ranges to compare' if a.runs < 2 else 'the ranges overlap' if overlap else
                   'this commit is faster' if lo > max(rows['parent']) else 'this commit is SLOWER: the ranges separate'}
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('leg', choices=['untagged', 'cost'])
  ap.add_argument('--parent', default=None, help='untagged: a built checkout of the parent commit')
  ap.add_argument('--runs', type=int, default=5)
  ap.add_argument('--configs', type=lambda v: [int(x) for x in v.split(',')], default=[2, 4, 1, 3],
                  help='untagged: the BASELINE configs to measure (a long session may be split over several calls)')
  ap.add_argument('--steps', type=int, default=3)
  ap.add_argument('--warmup', type=int, default=1)
  ap.add_argument('--frames', type=int, default=500)
  ap.add_argument('--utterances', type=int, default=64)
  ap.add_argument('--out', default=os.path.join(_ROOT, 'profiles', 'known_rate.json'))
  a = ap.parse_args()
  if a.leg == 'untagged':
    res = leg_untagged(a)
  else:
    params = weights.load_checkpoint(os.path.join(score_rate.GOLDEN, 'trained_d256.uisrnn'))
    res = {'cost': leg_cost(params, a)}
  print(json.dumps(res), flush=True)
  old = {}
  if os.path.exists(a.out):
    with open(a.out) as f:
      old = json.load(f)
  old.update(res)
  os.makedirs(os.path.dirname(a.out), exist_ok=True)
  with open(a.out, 'w') as f:
    json.dump(old, f, indent=1)


if __name__ == '__main__':
  main()
