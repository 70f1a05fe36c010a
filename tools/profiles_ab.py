"""The existing scoring calls and the benchmark line, the parent commit against this tree, in one sitting.

  python tools/profiles_ab.py --parent DIR [--runs 5] [--out profiles/profiles_ab.json]

DIR is a checkout of the parent commit with its library built in place (`python -m uisrnn_amd.build` there).  Each
tree's tools import that tree's own package and load that tree's own library, so the two sides share nothing but the
device.  Per figure `--runs` process runs of each side, alternating parent / tree:

  tools/score_rate.py --quick                      score_ms of its 64 x 500 line
  bench.py --gpus 1 --steps 10 --warmup 3          ms_per_step and frames/s of configs[1]
  tools/speakers_rate.py --steps 4                 uis_score_speakers wall / device ms at 64 x 500 and 1024 x 1000

The rule (DESIGN.md sections 21 and 32): every run of this tree lies under the parent's maximum plus the parent's own
spread (max - min).  The file holds every run, the bound and the verdict per figure.
"""

import argparse
import json
import os
import subprocess
import sys
import tempfile

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = ['bench.py', '--gpus', '1', '--steps', '10', '--warmup', '3', '--no_cpu_baseline', '--no_extra_configs', '--no_host_buffers']


def last_json_line(text):
  return json.loads([line for line in text.splitlines() if line.startswith('{')][-1])


def run(tree, argv):
  """One process run in `tree`; its standard output."""
  done = subprocess.run([sys.executable] + argv, cwd=tree, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=600)
  return done.stdout.decode()


def figures(kind, tree, tmp):
  """{figure: value} of one process run of `kind` in `tree`."""
  if kind == 'score':
    line = last_json_line(run(tree, ['tools/score_rate.py', '--quick', '--out', os.path.join(tmp, 'score.json')]))
    return {'score_rate_quick_score_ms': line['score_ms']}
  if kind == 'bench':
    line = last_json_line(run(tree, BENCH))
    return {'bench_ms_per_step': line['ms_per_step'], 'bench_frames_per_s': line['value']}
  out = os.path.join(tmp, 'speakers.json')
  run(tree, ['tools/speakers_rate.py', '--steps', '4', '--out', out])
  with open(out) as f:
    res = json.load(f)
  return {'speakers_rate_{}_{}'.format(batch, key): res[batch]['score_speakers'][key]
          for batch in ('64x500', '1024x1000') for key in ('wall_ms', 'device_ms')}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--parent', required=True, help='a checkout of the parent commit, its library built')
  ap.add_argument('--runs', type=int, default=5)
  ap.add_argument('--out', default=os.path.join(_ROOT, 'profiles', 'profiles_ab.json'))
  a = ap.parse_args()
  trees = {'parent': os.path.abspath(a.parent), 'tree': _ROOT}
  res = {}
  with tempfile.TemporaryDirectory() as tmp:
    for kind in ('score', 'bench', 'speakers'):
      for _ in range(a.runs):
        for side, tree in trees.items():   # (alternating: both sides see the same clocks and neighbours)
          for name, value in figures(kind, tree, tmp).items():
            res.setdefault('{}_{}'.format(name, side), []).append(value)
      print(kind, 'done', flush=True)
  rule = {}
  for key in sorted(k[:-len('_parent')] for k in res if k.endswith('_parent')):
    if key == 'bench_frames_per_s':   # (higher is better: reported, held through ms_per_step)
      continue
    parent, tree = res[key + '_parent'], res[key + '_tree']
    bound = max(parent) + (max(parent) - min(parent))
    rule[key] = {'bound': bound, 'tree_max': max(tree), 'within': all(v <= bound for v in tree)}
    print('{:<36} parent [{:.3f}, {:.3f}] tree [{:.3f}, {:.3f}] bound {:.3f} {}'.format(
        key, min(parent), max(parent), min(tree), max(tree), bound, 'within' if rule[key]['within'] else 'OVER'))
  res['rule'] = rule
  res['note'] = '{} alternating process runs each, one sitting'.format(a.runs)
  os.makedirs(os.path.dirname(a.out), exist_ok=True)
  with open(a.out, 'w') as f:
    json.dump(res, f, indent=1)
  print('wrote', a.out)


if __name__ == '__main__':
  main()
