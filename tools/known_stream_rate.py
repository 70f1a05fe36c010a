"""What known speakers in streaming sessions cost on the MI355X.  Nothing here is a threshold: the
figures are recorded, losses included.

  python tools/known_stream_rate.py --parent DIR [--runs 5] [--out profiles/known_stream_rate.json]

A 64-slot session on trained_d256, beam 10, synthetic utterances (uisrnn_amd.synth).  Every leg is a process of its own
(one handle, one session), this tree and a built checkout of the parent commit (--parent) interleaved, --runs each:
  untagged   one frame per push (--frames pushes) and 16 frames per push, no table: microseconds per push, this commit
             against the parent commit; the two ranges and whether they overlap
  tagged     the same two shapes with every third frame tagged (tests/known_ref.py's pattern), this commit only,
             against this commit's untagged legs
  calls      on the state the one-frame leg leaves: uis_stream_bindings (device and per-call time) beside
             uis_stream_nbest(1) (per-call time: it prints no trace line); uis_stream_retire's query (device and per-call
             time), this commit against the parent commit
The worker below uses nothing but the session calls both commits have, except where a leg is this commit's alone.
"""

import argparse
import json
import os
import subprocess
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_WORKER = r'''
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
from uisrnn_amd import _capi, synth, weights
frames, per_push, tagged, calls = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3] == '1', sys.argv[4] == '1'
U = 64
params = weights.load_checkpoint(os.path.join('tests', 'golden', 'trained_d256.uisrnn'))
dim = int(params['observation_dim'])
x = np.stack([synth.make_utterance(7000 + u, frames, dim)[0] for u in range(U)]).astype(np.float32)
tags = np.array([[((t + u) // 5) % 3 + 1 if (t + u) % 3 == 0 else 0 for t in range(frames)] for u in range(U)], dtype=np.uint8)
dec = _capi.Decoder(params)
dec.stream_begin(U, 10, frames, max_clusters=16)
res = {}
try:
  extra = (lambda t: {'speakers': np.ascontiguousarray(tags[:, t:t + per_push]).reshape(-1)}) if tagged else (lambda t: {})
  dec.stream_push(x[:, :per_push], **extra(0))   # (the first push: allocations, the cooperative launch's check)
  t0 = time.perf_counter()
  n = 0
  for t in range(per_push, frames - per_push + 1, per_push):
    dec.stream_push(x[:, t:t + per_push], **extra(t))
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
    res['nbest_1_us_per_call'] = per_call(lambda: dec.stream_nbest(1))
    os.environ['UIS_RETIRE_TRACE'] = '1'
    res['retire_query_us_per_call'] = per_call(lambda: dec.stream_retire(clusters=[None] * U))
    os.environ.pop('UIS_RETIRE_TRACE')
    if hasattr(dec, 'stream_bindings'):
      os.environ['UIS_BINDINGS_TRACE'] = '1'
      res['bindings_us_per_call'] = per_call(dec.stream_bindings)
      os.environ.pop('UIS_BINDINGS_TRACE')
      res['bound_tags'] = int(dec.stream_bindings()[:, 0].sum())
finally:
  dec.stream_end()
  dec.close()
print('RESULT ' + json.dumps(res), flush=True)
'''


def _median(values):
  values = sorted(values)
  return values[len(values) // 2] if values else None


def _worker(tree, frames, per_push, tagged, calls):
  done = subprocess.run([sys.executable, '-c', _WORKER, str(frames), str(per_push), '1' if tagged else '0', '1' if calls else '0'],
                        cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True, timeout=300)
  res = json.loads([l for l in done.stdout.decode().splitlines() if l.startswith('RESULT ')][-1][7:])
  err = done.stderr.decode().splitlines()
  for call, key in (('uis_stream_retire:', 'retire_query_device_us'), ('uis_stream_bindings:', 'bindings_device_us')):
    ms = [float(l.split('device_ms ')[1].split()[0]) for l in err if l.startswith(call) and 'device_ms ' in l]
    if ms:
      res[key] = 1e3 * _median(ms)
  return res


def _verdict(this, parent):
  lo, hi = min(this), max(this)
  if hi >= min(parent) and lo <= max(parent):
    return 'the ranges overlap'
  return 'this commit is faster' if hi < min(parent) else 'this commit is SLOWER: the ranges separate'


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--parent', required=True, help='a built checkout of the parent commit')
  ap.add_argument('--runs', type=int, default=5)
  ap.add_argument('--frames', type=int, default=320)
  ap.add_argument('--out', default=os.path.join(_ROOT, 'profiles', 'known_stream_rate.json'))
  a = ap.parse_args()
  if not os.path.exists(os.path.join(a.parent, 'uisrnn_amd', '_capi.py')):
    raise SystemExit('--parent: a checkout of the parent commit with its library built')
  res = {'how': '64 slots, trained_d256, beam 10, %d frames per slot; one process per leg, the parent commit and this one '
                'interleaved, %d runs each; microseconds' % (a.frames, a.runs)}
  for per_push in (1, 16):
    rows = {'parent_untagged': [], 'this_untagged': [], 'this_tagged': []}
    call_rows = {}
    for _ in range(a.runs):
      for key, tree, tagged in (('parent_untagged', a.parent, False), ('this_untagged', _ROOT, False), ('this_tagged', _ROOT, True)):
        out = _worker(tree, a.frames, per_push, tagged, calls=per_push == 1)
        rows[key].append(out['us_per_push'])
        for k, v in out.items():
          if k not in ('us_per_push', 'pushes'):
            call_rows.setdefault(key + '_' + k, []).append(v)
        print(per_push, key, out, flush=True)
    leg = {'us_per_push': rows, 'untagged_this_commit_against_the_parent': _verdict(rows['this_untagged'], rows['parent_untagged']),
           'tagged_against_untagged_this_commit': _verdict(rows['this_tagged'], rows['this_untagged']),
           'median_us_per_push': {k: _median(v) for k, v in rows.items()}}
    if call_rows:
      leg['calls_on_the_final_state'] = {k: {'median': _median(v), 'min': min(v), 'max': max(v)} for k, v in sorted(call_rows.items())}
      leg['retire_query_this_commit_against_the_parent'] = _verdict(call_rows['this_untagged_retire_query_us_per_call'],
                                                                     call_rows['parent_untagged_retire_query_us_per_call'])
    res['%d_frames_per_push' % per_push] = leg
  print(json.dumps(res), flush=True)
  os.makedirs(os.path.dirname(a.out), exist_ok=True)
  with open(a.out, 'w') as f:
    json.dump(res, f, indent=1)


if __name__ == '__main__':
  main()
