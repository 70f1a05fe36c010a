"""What a speaker bound (max_speakers) buys on the MI355X.  Nothing here is a threshold: the
figures are recorded, losses included.

  python tools/limit_rate.py wide     [--frames 500] [--steps 3] [--out profiles/limit_rate.json]
  python tools/limit_rate.py policy   [--frames 500] [--steps 3]
  python tools/limit_rate.py service  [--frames 600]
  python tools/limit_rate.py unbounded --parent DIR [--runs 5]

trained_d256, synthetic utterances (uisrnn_amd.synth), 64 utterances.
  wide     configs[2]'s shape (beam 50, look_ahead 2, test_iteration 2): predict with max_speakers=4 against the
           unbounded predict at configs[2]'s cap 12 (its compile-time shape class), and under max_clusters=4; median
           wall time per call, the kernel family and the cluster cap each starts with.
  policy   beam 50 / look_ahead 1 under max_speakers=4: with the cap policy (the decode starts at cap 4 and stays on the
           fast select) and without it (max_clusters=16 given, which the policy leaves alone), and the unbounded decode.
  service  an endless 64-slot session over streams that walk through thirty speakers each (window 64, horizon 32,
           one frame per push, max_clusters 16): model.online(..., max_speakers=8) against the same service with
           retire_at=12; pushes per second, the push a service stops at, the utterances at the cap at the end.
  unbounded  what the unbounded decode pays for the feature: bench.py --gpus 1 at configs 1 and 3, this tree and a built
           checkout of the parent commit (--parent) interleaved in one session, --runs each; the two ranges of frames/s
           and whether they overlap.
Every leg merges its keys into --out.
"""

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, 'tools'))

import score_rate  # noqa: E402  pylint: disable=wrong-import-position
import uisrnn_amd  # noqa: E402  pylint: disable=wrong-import-position
from uisrnn_amd import synth, weights  # noqa: E402  pylint: disable=wrong-import-position
from uisrnn_amd import uisrnn as host  # noqa: E402  pylint: disable=wrong-import-position


def _model(params, beam, look_ahead, test_iteration):
  dim = int(params['observation_dim'])
  model_args, _, args = uisrnn_amd.parse_arguments(
      ['--observation_dim', str(dim), '--rnn_hidden_size', str(int(params['rnn_hidden_size']))])
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params)
  args.beam_size, args.look_ahead, args.test_iteration = beam, look_ahead, test_iteration
  return model, args


def _timed(model, seqs, args, steps, warmup, **kwargs):
  times = []
  for k in range(warmup + steps):
    t0 = time.perf_counter()
    labels = model.predict(seqs, args, **kwargs)
    if k >= warmup:
      times.append(time.perf_counter() - t0)
  frames = sum(s.shape[0] for s in seqs)
  ms = 1e3 * float(np.median(times))
  limits = host._check_max_speakers(kwargs.get('max_speakers'), args, len(seqs))  # pylint: disable=protected-access
  return {'ms_per_call': ms, 'frames_per_s': frames / (ms / 1e3), 'decode_kernel': model.last_stats['decode_kernel'],
          'device_ms': model.last_stats['decode_ms'], 'first_cap': host._initial_cluster_cap(args, limits),  # pylint: disable=protected-access
          'single_pass': bool(model._single_pass),  # pylint: disable=protected-access
          'speakers_found': int(max(max(l) for l in labels if l) + 1)}


def leg_wide(params, a):
  model, args = _model(params, 50, 2, 2)
  seqs = [synth.make_utterance(7000 + u, a.frames, int(params['observation_dim']))[0] for u in range(a.utterances)]
  args.max_clusters = 12   # configs[2]'s own cap
  res = {'utterances': a.utterances, 'frames': a.frames, 'beam': 50, 'look_ahead': 2, 'test_iteration': 2,
         'unbounded_cap_12': _timed(model, seqs, args, a.steps, a.warmup),
         'max_speakers_4_cap_12': _timed(model, seqs, args, a.steps, a.warmup, max_speakers=4)}
  args.max_clusters = 4
  res['max_speakers_4_cap_4'] = _timed(model, seqs, args, a.steps, a.warmup, max_speakers=4)
  return res


def leg_policy(params, a):
  model, args = _model(params, 50, 1, 2)
  seqs = [synth.make_utterance(7000 + u, a.frames, int(params['observation_dim']))[0] for u in range(a.utterances)]
  res = {'utterances': a.utterances, 'frames': a.frames, 'beam': 50, 'look_ahead': 1, 'test_iteration': 2,
         'unbounded': _timed(model, seqs, args, a.steps, a.warmup),
         'max_speakers_4_with_the_policy': _timed(model, seqs, args, a.steps, a.warmup, max_speakers=4)}
  args.max_clusters = 16
  res['max_speakers_4_without_the_policy'] = _timed(model, seqs, args, a.steps, a.warmup, max_speakers=4)
  return res


def _service(model, args, x, **kwargs):
  n_utt, n = x.shape[0], x.shape[1]
  with model.online(n_utt, args, 64, horizon=32, **kwargs) as session:
    t0 = time.perf_counter()
    stopped, pushed = None, 0
    try:
      for t in range(n):
        session.push(x[:, t:t + 1])
        pushed += 1
    except (RuntimeError, ValueError) as err:   # (reported, not hidden: tools/retire_rate.py)
      stopped = str(err)
    total = time.perf_counter() - t0
    _, _, overflow, _ = session._decoder.stream_labels()  # pylint: disable=protected-access
    counts = [k for k, _ in session.cluster_counts()]
  n = max(pushed, 1)
  return {'pushes_per_s': n / total, 'us_per_push': 1e6 * total / n, 'pushes': pushed, 'stopped_by': stopped,
          'utterances_at_the_cap': int((overflow != 0).sum()), 'largest_cluster_count': int(max(counts))}


def leg_service(params, a):
  model, args = _model(params, 10, 1, 1)
  args.max_clusters = 16
  dim = int(params['observation_dim'])
  x = np.stack([synth.make_utterance(7000 + u, a.frames, dim, num_speakers=30, mean_segment=10.0)[0]
                for u in range(a.utterances)])
  return {'utterances': a.utterances, 'frames': a.frames, 'window': 64, 'horizon': 32, 'beam': 10, 'max_clusters': 16,
          'max_speakers_8': _service(model, args, x, max_speakers=8),
          'retire_at_12': _service(model, args, x, retire_at=12),
          'neither': _service(model, args, x)}


def _bench(tree, config, steps):
  out = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(steps), '--warmup', '2', '--config',
                        str(config), '--no_cpu_baseline', '--no_extra_configs', '--no_host_buffers'],
                       cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True, timeout=300).stdout
  return float(json.loads(out.decode().strip().splitlines()[-1])['value'])


def leg_unbounded(a):
  if not a.parent or not os.path.exists(os.path.join(a.parent, 'bench.py')):
    raise SystemExit('--parent: a checkout of the parent commit with its library built')
  res = {'how': 'bench.py --gpus 1 --warmup 2 --no_cpu_baseline --no_extra_configs --no_host_buffers; the parent commit '
                'and this one interleaved in one session', 'runs_each': a.runs}
  for config, steps in ((1, 10), (3, 3)):
    rows = {'parent': [], 'this_commit': []}
    for _ in range(a.runs):
      rows['parent'].append(_bench(a.parent, config, steps))
      rows['this_commit'].append(_bench(_ROOT, config, steps))
      print(config, rows['parent'][-1], rows['this_commit'][-1], flush=True)
    lo, hi = min(rows['this_commit']), max(rows['this_commit'])
    overlap = hi >= min(rows['parent']) and lo <= max(rows['parent'])
    res['config_%d' % config] = {
        'steps': steps, 'frames_per_s': rows,
        'verdict': 'the ranges overlap' if overlap else
                   'this commit is faster' if lo > max(rows['parent']) else 'this commit is SLOWER: the ranges separate'}
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('leg', choices=['wide', 'policy', 'service', 'unbounded'])
  ap.add_argument('--parent', default=None, help='unbounded: a built checkout of the parent commit')
  ap.add_argument('--runs', type=int, default=5)
  ap.add_argument('--steps', type=int, default=3)
  ap.add_argument('--warmup', type=int, default=1)
  ap.add_argument('--frames', type=int, default=500)
  ap.add_argument('--utterances', type=int, default=64)
  ap.add_argument('--out', default=os.path.join(_ROOT, 'profiles', 'limit_rate.json'))
  a = ap.parse_args()
  if a.leg == 'unbounded':
    res = {'unbounded_against_the_parent_commit': leg_unbounded(a)}
  else:
    params = weights.load_checkpoint(os.path.join(score_rate.GOLDEN, 'trained_d256.uisrnn'))
    res = {a.leg: {'wide': leg_wide, 'policy': leg_policy, 'service': leg_service}[a.leg](params, a)}
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
