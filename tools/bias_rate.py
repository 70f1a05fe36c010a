"""What the per-frame transition_bias costs on the MI355X.  Nothing here is a threshold: the
figures are recorded, losses included.

  python tools/bias_rate.py unbiased --parent DIR [--runs 5] [--configs 2,4,1,3] [--out profiles/bias_rate.json]
  python tools/bias_rate.py cost     [--frames 500] [--steps 3]
  python tools/bias_rate.py score    [--frames 500] [--steps 3]
  python tools/bias_rate.py session  [--frames 300]

trained_d256, synthetic utterances (uisrnn_amd.synth), 64 utterances.
  unbiased  what the decode without a table pays for the feature: bench.py --gpus 1 at configs 2 and 4 (whose kernels the
            rule touches) and 1 and 3 (which it must not), this tree and a built checkout of the parent commit (--parent)
            interleaved in one session, --runs each; the two ranges of frames/s and whether they overlap.
  cost      64 x --frames, beam 10, test_iteration 2 (configs[1]'s shape): the decode under a table (k_decode_resident)
            against the decode without one (k_decode_rs), and against the decode without one under
            UIS_FLAG_OWNER_SELECT (the same kernel: the rule plus the table's upload); configs[2]'s shape (beam 50,
            look_ahead 2) with and without a table.  Device milliseconds and wall time per call.
  score     score_labels with and without a table.
  session   a 64-slot session, one frame per push, with and without a per-push table: pushes per second.
The table: a speaker-change detector's shape -- 0.5 at every tenth frame, 0 inside "words" (three frames in ten), NaN
elsewhere.  Every leg merges its keys into --out.
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
from uisrnn_amd import _capi, synth, weights  # noqa: E402  pylint: disable=wrong-import-position


def _table(n, u=0):
  b = np.full(n, np.nan)
  t = np.arange(n) + u
  b[t % 10 == 0] = 0.5
  b[(t % 10 >= 4) & (t % 10 <= 6)] = 0.0
  if n and b[0] == 0.0:
    b[0] = np.nan
  return b


def _seqs(params, a):
  return [synth.make_utterance(7000 + u, a.frames, int(params['observation_dim']))[0] for u in range(a.utterances)]


def _timed_decode(dec, seqs, beam, look_ahead, tau, steps, warmup, cap=0, flags=0, bias=None):
  wall, dev = [], []
  for k in range(warmup + steps):
    t0 = time.perf_counter()
    out = dec.decode_f64(seqs, beam, look_ahead, tau, max_clusters=cap, flags=flags, bias=bias)
    if k >= warmup:
      wall.append(time.perf_counter() - t0)
      dev.append(out['stats']['decode_ms'])
  frames = sum(s.shape[0] for s in seqs)
  return {'ms_per_call': 1e3 * float(np.median(wall)), 'device_ms': float(np.median(dev)),
          'frames_per_s_device': frames / (float(np.median(dev)) / 1e3), 'decode_kernel': out['stats']['decode_kernel'],
          'instantiation': list(dec.last_instantiation()), 'overflow': int(out['overflow'].any())}


def leg_cost(params, a):
  seqs = _seqs(params, a)
  bias = np.concatenate([_table(len(s), u) for u, s in enumerate(seqs)])
  dec = _capi.Decoder(params)
  try:
    res = {'utterances': a.utterances, 'frames': a.frames, 'beam': 10, 'test_iteration': 2,
           'no_table': _timed_decode(dec, seqs, 10, 1, 2, a.steps, a.warmup),
           'no_table_owner_select': _timed_decode(dec, seqs, 10, 1, 2, a.steps, a.warmup, flags=_capi.UIS_FLAG_OWNER_SELECT),
           'table': _timed_decode(dec, seqs, 10, 1, 2, a.steps, a.warmup, bias=bias),
           'configs2_shape_no_table': _timed_decode(dec, seqs, 50, 2, 2, a.steps, a.warmup, cap=12),
           'configs2_shape_table': _timed_decode(dec, seqs, 50, 2, 2, a.steps, a.warmup, cap=12, bias=bias)}
  finally:
    dec.close()
  return res


def leg_score(params, a):
  seqs = _seqs(params, a)
  dim = int(params['observation_dim'])
  model_args, _, args = uisrnn_amd.parse_arguments(
      ['--observation_dim', str(dim), '--rnn_hidden_size', str(int(params['rnn_hidden_size']))])
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params)
  args.beam_size, args.look_ahead, args.test_iteration = 10, 1, 1
  labels = model.predict(seqs, args)
  tables = [_table(len(s), u) for u, s in enumerate(seqs)]
  res = {'utterances': a.utterances, 'frames': a.frames}
  for name, kw in (('no_table', {}), ('table', {'transition_bias': tables})):
    times = []
    for k in range(a.warmup + a.steps):
      t0 = time.perf_counter()
      model.score_labels(seqs, labels, **kw)
      if k >= a.warmup:
        times.append(time.perf_counter() - t0)
    res[name] = {'ms_per_call': 1e3 * float(np.median(times))}
  return res


def leg_session(params, a):
  dim = int(params['observation_dim'])
  x = np.stack([synth.make_utterance(7000 + u, a.frames, dim)[0] for u in range(a.utterances)]).astype(np.float32)
  tables = np.stack([_table(a.frames, u) for u in range(a.utterances)])
  res = {'utterances': a.utterances, 'frames': a.frames, 'beam': 10, 'one_frame_per_push': True}
  dec = _capi.Decoder(params)
  try:
    for name, biased in (('no_table', False), ('table', True), ('no_table_again', False)):
      dec.stream_begin(a.utterances, 10, a.frames, max_clusters=16)
      try:
        t0 = time.perf_counter()
        for t in range(a.frames):
          dec.stream_push(x[:, t:t + 1], bias=tables[:, t] if biased else None)
        total = time.perf_counter() - t0
      finally:
        dec.stream_end()
      res[name] = {'pushes_per_s': a.frames / total, 'us_per_push': 1e6 * total / a.frames}
  finally:
    dec.close()
  return res


def _bench(tree, config, steps):
  out = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(steps), '--warmup', '2', '--config',
                        str(config), '--no_cpu_baseline', '--no_extra_configs', '--no_host_buffers'],
                       cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True, timeout=300).stdout
  return float(json.loads(out.decode().strip().splitlines()[-1])['value'])


def leg_unbiased(a):
  if not a.parent or not os.path.exists(os.path.join(a.parent, 'bench.py')):
    raise SystemExit('--parent: a checkout of the parent commit with its library built')
  res = {'how': 'bench.py --gpus 1 --warmup 2 --no_cpu_baseline --no_extra_configs --no_host_buffers; the parent commit '
                'and this one interleaved in one session', 'runs_each': a.runs}
  for config, steps in ((2, 3), (4, 3), (1, 10), (3, 3)):
    if config not in a.configs:
      continue
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
  ap.add_argument('leg', choices=['unbiased', 'cost', 'score', 'session'])
  ap.add_argument('--parent', default=None, help='unbiased: a built checkout of the parent commit')
  ap.add_argument('--runs', type=int, default=5)
  ap.add_argument('--configs', type=lambda v: [int(x) for x in v.split(',')], default=[2, 4, 1, 3],
                  help='unbiased: the BASELINE configs to measure (a long session may be split over several calls)')
  ap.add_argument('--steps', type=int, default=3)
  ap.add_argument('--warmup', type=int, default=1)
  ap.add_argument('--frames', type=int, default=500)
  ap.add_argument('--utterances', type=int, default=64)
  ap.add_argument('--out', default=os.path.join(_ROOT, 'profiles', 'bias_rate.json'))
  a = ap.parse_args()
  if a.leg == 'unbiased':
    res = {'unbiased_against_the_parent_commit_configs_%s' % '_'.join(str(c) for c in a.configs): leg_unbiased(a)}
  else:
    params = weights.load_checkpoint(os.path.join(score_rate.GOLDEN, 'trained_d256.uisrnn'))
    res = {a.leg: {'cost': leg_cost, 'score': leg_score, 'session': leg_session}[a.leg](params, a)}
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
