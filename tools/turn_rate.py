"""What the minimum turn length costs on the MI355X.  Nothing here is a threshold: the figures
are recorded, losses included.

  python tools/turn_rate.py untouched --parent DIR [--runs 5] [--configs 2,4,1,3] [--out profiles/turn_rate.json]
  python tools/turn_rate.py cost      [--frames 500] [--steps 3] [--min_turn 3]

trained_d256, synthetic utterances (uisrnn_amd.synth), 64 utterances.
  untouched  what the decode without a table pays for the feature: bench.py --gpus 1 at configs 2 and 4 (whose selects
             the rule touches) and 1 and 3 (which it must not), this tree and a built checkout of the parent commit
             (--parent) interleaved in one session: --runs each at configs 2 and 4, one pair at configs 1 and 3; the
             two ranges of frames/s and whether they overlap.
  cost       64 x --frames, beam 10, test_iteration 2 (configs[1]'s shape): the decode under m = --min_turn on every
             utterance (k_decode_resident) against the decode without a table (k_decode_rs: the planner exclusion), and
             against the decode without one under UIS_FLAG_OWNER_SELECT (the same kernel: the rule plus the upload).
             Device milliseconds and wall time per call, and how many completed turns shorter than m the decode without
             a table returns, and the rnn rows of one decode of each leg.
Every leg merges its keys into --out.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, 'tools'))

import bias_rate  # noqa: E402  pylint: disable=wrong-import-position
import score_rate  # noqa: E402  pylint: disable=wrong-import-position
from uisrnn_amd import _capi, synth, weights  # noqa: E402  pylint: disable=wrong-import-position


def _short_turns(labels, lengths, m):
  """Completed turns shorter than m in the packed labels of utterances of `lengths` frames."""
  short, at = 0, 0
  for n in lengths:
    lab = labels[at:at + n]
    at += n
    edges = np.flatnonzero(np.diff(lab)) + 1
    runs = np.diff(np.concatenate([[0], edges]))   # (every turn but the last)
    short += int((runs < m).sum())
  return short


def _timed_decode(dec, seqs, steps, warmup, m, flags=0, min_turn=None):
  wall, dev = [], []
  for k in range(warmup + steps):
    t0 = time.perf_counter()
    out = dec.decode_f64(seqs, 10, 1, 2, flags=flags, min_turn=min_turn)
    if k >= warmup:
      wall.append(time.perf_counter() - t0)
      dev.append(out['stats']['decode_ms'])
  frames = sum(s.shape[0] for s in seqs)
  return {'ms_per_call': 1e3 * float(np.median(wall)), 'device_ms': float(np.median(dev)),
          'frames_per_s_device': frames / (float(np.median(dev)) / 1e3), 'decode_kernel': out['stats']['decode_kernel'],
          'instantiation': list(dec.last_instantiation()), 'overflow': int(out['overflow'].any()),
          'speakers_found': int(max(out['labels'].max(), -1)) + 1, 'rnn_rows': int(out['stats']['rnn_rows']),
          'completed_turns_shorter_than_m': _short_turns(out['labels'], [s.shape[0] for s in seqs], m)}


def leg_cost(params, a):
  seqs = [synth.make_utterance(7000 + u, a.frames, int(params['observation_dim']))[0] for u in range(a.utterances)]
  table = [a.min_turn] * a.utterances
  dec = _capi.Decoder(params)
  try:
    res = {'utterances': a.utterances, 'frames': a.frames, 'beam': 10, 'test_iteration': 2, 'min_turn': a.min_turn,
           'no_table': _timed_decode(dec, seqs, a.steps, a.warmup, a.min_turn),
           'no_table_owner_select': _timed_decode(dec, seqs, a.steps, a.warmup, a.min_turn, flags=_capi.UIS_FLAG_OWNER_SELECT),
           'table': _timed_decode(dec, seqs, a.steps, a.warmup, a.min_turn, min_turn=table)}
  finally:
    dec.close()
  return res


_TOUCHED = (2, 4)   # configs whose selects the rule's code sits in: --runs runs each; the others: one pair


def leg_untouched(a):
  if not a.parent or not os.path.exists(os.path.join(a.parent, 'bench.py')):
    raise SystemExit('--parent: a checkout of the parent commit with its library built')
  how = ('bench.py --gpus 1 --warmup 2 --no_cpu_baseline --no_extra_configs --no_host_buffers; the parent commit and '
         'this one interleaved in one session')
  res = {}   # (one key per config: a later session of the same config replaces it, whatever else it measured)
  for config, steps in ((2, 3), (4, 3), (1, 10), (3, 3)):
    if config not in a.configs:
      continue
    runs = a.runs if config in _TOUCHED else 1
    rows = {'parent': [], 'this_commit': []}
    for _ in range(runs):
      rows['parent'].append(bias_rate._bench(a.parent, config, steps))  # pylint: disable=protected-access
      rows['this_commit'].append(bias_rate._bench(_ROOT, config, steps))  # pylint: disable=protected-access
      print(config, rows['parent'][-1], rows['this_commit'][-1], flush=True)
    lo, hi = min(rows['this_commit']), max(rows['this_commit'])
    overlap = hi >= min(rows['parent']) and lo <= max(rows['parent'])
    res['no_table_against_the_parent_commit_config_%d' % config] = {
        'how': how, 'runs_each': runs, 'steps': steps, 'frames_per_s': rows,
        'verdict': 'one pair of runs: no ranges to compare' if runs < 2 else 'the ranges overlap' if overlap else
                   'this commit is faster' if lo > max(rows['parent']) else 'this commit is SLOWER: the ranges separate'}
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('leg', choices=['untouched', 'cost'])
  ap.add_argument('--parent', default=None, help='untouched: a built checkout of the parent commit')
  ap.add_argument('--runs', type=int, default=5)
  ap.add_argument('--configs', type=lambda v: [int(x) for x in v.split(',')], default=[2, 4, 1, 3],
                  help='untouched: the BASELINE configs to measure (a long session may be split over several calls)')
  ap.add_argument('--steps', type=int, default=3)
  ap.add_argument('--warmup', type=int, default=1)
  ap.add_argument('--frames', type=int, default=500)
  ap.add_argument('--utterances', type=int, default=64)
  ap.add_argument('--min_turn', type=int, default=3)
  ap.add_argument('--out', default=os.path.join(_ROOT, 'profiles', 'turn_rate.json'))
  a = ap.parse_args()
  if a.leg == 'untouched':
    res = leg_untouched(a)
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
