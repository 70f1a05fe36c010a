"""What a minimum turn length in streaming sessions costs on the MI355X.  Nothing here is a
threshold: the figures are recorded, losses included.

  python tools/turn_stream_rate.py --parent DIR [--runs 5] [--legs push,bench] [--out profiles/turn_stream_rate.json]

push   a 64-slot session on trained_d256, beam 10, synthetic utterances (uisrnn_amd.synth).  Every leg is a process of
       its own (one handle, one session), this tree and a built checkout of the parent commit (--parent) interleaved,
       --runs each:
         no rule     one frame per push (--frames pushes) and 16 frames per push: microseconds per push, this commit
                     against the parent commit; the two ranges and whether they overlap -- the one condition
         m = 3       the same two shapes with every slot under m = 3, this commit only
         persistent  one frame per push in a UIS_FLAG_PERSISTENT session, without a rule and under m = 3
         calls       on the state the one-frame leg leaves: uis_session_turns (device and per-call time) beside
                     uis_stream_nbest(1); uis_stream_retire's query (device and per-call time) without a rule -- this
                     commit against the parent -- and under m = 3
         turns       completed turns shorter than 3 frames in the labels of the one-frame leg, without and under m = 3
bench  bench.py --gpus 1 at every BASELINE config, one pair of runs per config (tools/bias_rate.py's invocation)
The worker uses nothing but the session calls both commits have, except where a leg is this commit's alone.
"""

import argparse
import json
import os
import subprocess
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, 'tools'))

_WORKER = r'''
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
from uisrnn_amd import _capi, synth, weights
frames, per_push, m, calls, persistent = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4] == '1', sys.argv[5] == '1'
U = 64
params = weights.load_checkpoint(os.path.join('tests', 'golden', 'trained_d256.uisrnn'))
dim = int(params['observation_dim'])
x = np.stack([synth.make_utterance(7000 + u, frames, dim)[0] for u in range(U)]).astype(np.float32)
dec = _capi.Decoder(params)
try:
  dec.stream_begin(U, 10, frames, max_clusters=16, flags=_capi.UIS_FLAG_PERSISTENT if persistent else 0)
except _capi.HipLibraryError as err:   # (a device that is not whole: the leg is recorded as not run)
  if not persistent or err.status != _capi.UIS_ERR_UNSUPPORTED:
    raise
  print('RESULT ' + json.dumps({'unsupported': True}), flush=True)
  dec.close()
  sys.exit(0)
res = {}
try:
  if m:
    dec.session_set_min_turn([m] * U)
  dec.stream_push(x[:, :per_push])   # (the first push: allocations, the cooperative launch's check)
  t0 = time.perf_counter()
  n = 0
  for t in range(per_push, frames - per_push + 1, per_push):
    dec.stream_push(x[:, t:t + per_push])
    n += 1
  res['us_per_push'] = 1e6 * (time.perf_counter() - t0) / n
  res['pushes'] = n
  if calls:
    def per_call(f, reps=50):
      f()
      t0 = time.perf_counter()
      for _ in range(reps):
        f()
      return 1e6 * (time.perf_counter() - t0) / reps
    labels = dec.stream_labels()[0]
    short = total = 0
    for row in labels:
      row = row.tolist()
      cuts = [0] + [t for t in range(1, len(row)) if row[t] != row[t - 1]] + [len(row)]
      lens = [b - a for a, b in zip(cuts, cuts[1:])][:-1]   # (completed turns: all but the last)
      short += sum(1 for v in lens if v < 3)
      total += len(lens)
    res['completed_turns'] = total
    res['completed_turns_shorter_than_3'] = short
    res['nbest_1_us_per_call'] = per_call(lambda: dec.stream_nbest(1))
    os.environ['UIS_RETIRE_TRACE'] = '1'
    res['retire_query_us_per_call'] = per_call(lambda: dec.stream_retire(clusters=[None] * U))
    os.environ.pop('UIS_RETIRE_TRACE')
    if hasattr(dec, 'session_turns'):
      os.environ['UIS_TURNS_TRACE'] = '1'
      res['turns_us_per_call'] = per_call(dec.session_turns)
      os.environ.pop('UIS_TURNS_TRACE')
      res['held_slots'] = int((dec.session_turns()[:, 1] < m).sum()) if m else 0
finally:
  dec.stream_end()
  dec.close()
print('RESULT ' + json.dumps(res), flush=True)
'''


def _median(values):
  values = sorted(values)
  return values[len(values) // 2] if values else None


def _worker(tree, frames, per_push, m, calls, persistent=False):
  done = subprocess.run([sys.executable, '-c', _WORKER, str(frames), str(per_push), str(m), '1' if calls else '0',
                         '1' if persistent else '0'], cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True, timeout=300)
  res = json.loads([l for l in done.stdout.decode().splitlines() if l.startswith('RESULT ')][-1][7:])
  err = done.stderr.decode().splitlines()
  for call, key in (('uis_stream_retire:', 'retire_query_device_us'), ('uis_session_turns:', 'turns_device_us')):
    ms = [float(l.split('device_ms ')[1].split()[0]) for l in err if l.startswith(call) and 'device_ms ' in l]
    if ms:
      res[key] = 1e3 * _median(ms)
  return res


def _verdict(this, other, first='this commit'):
  lo, hi = min(this), max(this)
  if hi >= min(other) and lo <= max(other):
    return 'the ranges overlap'
  return first + (' is faster' if hi < min(other) else ' is SLOWER') + ': the ranges separate'


def leg_push(a):
  res = {'how': '64 slots, trained_d256, beam 10, %d frames per slot; one process per leg, the parent commit and this one '
                'interleaved, %d runs each; microseconds' % (a.frames, a.runs)}
  for per_push in (1, 16):
    legs = [('parent_no_rule', a.parent, 0, False), ('this_no_rule', _ROOT, 0, False), ('this_m3', _ROOT, 3, False)]
    if per_push == 1:
      legs += [('this_persistent_no_rule', _ROOT, 0, True), ('this_persistent_m3', _ROOT, 3, True)]
    rows = {key: [] for key, _, _, _ in legs}
    call_rows = {}
    for _ in range(a.runs):
      for key, tree, m, persistent in legs:
        out = _worker(tree, a.frames, per_push, m, calls=per_push == 1 and not persistent, persistent=persistent)
        if out.get('unsupported'):
          continue
        rows[key].append(out['us_per_push'])
        for k, v in out.items():
          if k not in ('us_per_push', 'pushes'):
            call_rows.setdefault(key + '_' + k, []).append(v)
        print(per_push, key, out, flush=True)
    leg = {'us_per_push': rows, 'no_rule_this_commit_against_the_parent': _verdict(rows['this_no_rule'], rows['parent_no_rule']),
           'm3_against_no_rule_this_commit': _verdict(rows['this_m3'], rows['this_no_rule'], 'the push under m = 3'),
           'median_us_per_push': {k: _median(v) for k, v in rows.items()},
           'legs_the_device_refused': sorted(k for k, v in rows.items() if not v)}
    if call_rows:
      leg['on_the_final_state'] = {k: {'median': _median(v), 'min': min(v), 'max': max(v)} for k, v in sorted(call_rows.items())}
      leg['retire_query_this_commit_against_the_parent'] = _verdict(call_rows['this_no_rule_retire_query_us_per_call'],
                                                                     call_rows['parent_no_rule_retire_query_us_per_call'])
    res['%d_frames_per_push' % per_push] = leg
  return {'push': res}


def leg_bench(a):
  import bias_rate  # pylint: disable=import-outside-toplevel
  res = {'how': 'bench.py --gpus 1 --warmup 2 --no_cpu_baseline --no_extra_configs --no_host_buffers; the parent commit and '
                'this one, one pair of runs per config; frames per second'}
  for config, steps in ((1, 10), (2, 3), (3, 3), (4, 3)):
    parent = bias_rate._bench(a.parent, config, steps)   # pylint: disable=protected-access
    this = bias_rate._bench(_ROOT, config, steps)        # pylint: disable=protected-access
    res['config_%d' % config] = {'parent': parent, 'this_commit': this, 'ratio': this / parent}
    print(config, parent, this, flush=True)
  return {'bench': res}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--parent', required=True, help='a built checkout of the parent commit')
  ap.add_argument('--runs', type=int, default=5)
  ap.add_argument('--frames', type=int, default=320)
  ap.add_argument('--legs', type=lambda v: v.split(','), default=['push', 'bench'])
  ap.add_argument('--out', default=os.path.join(_ROOT, 'profiles', 'turn_stream_rate.json'))
  a = ap.parse_args()
  a.parent = os.path.abspath(a.parent)
  if not os.path.exists(os.path.join(a.parent, 'uisrnn_amd', '_capi.py')):
    raise SystemExit('--parent: a checkout of the parent commit with its library built')
  res = {}
  if 'push' in a.legs:
    res.update(leg_push(a))
  if 'bench' in a.legs:
    res.update(leg_bench(a))
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
