"""What speaker profiles cost on the MI355X: uis_speaker_profiles beside uis_score_speakers on the same batch, and
uis_session_profiles beside uis_stream_bindings on a 64-slot session.

  python tools/profiles_rate.py [--steps 10] [--warmup 2] [--out profiles/profiles_rate.json]

The batches of tools/speakers_rate.py (trained_d256, truth labels, frames in one pinned buffer): 64 x 500 and
1024 x 1000 frames; width = the batch's largest cluster count (+ 1 for uis_score_speakers).  The calls alternate inside
one process, uis_score_labels with them; per call the median wall time of `--steps` blocking calls after `--warmup` and
the median of the library's own device time (UIS_SCORE_TIMING=1: events around the kernels, copies excluded).

The session: 64 slots, beam 10, 40 frames pushed to each; uis_session_profiles and uis_stream_bindings alternate, wall
time and the device time of their trace lines (UIS_PROFILES_TRACE / UIS_BINDINGS_TRACE).

Then the 64 x 500 uis_speaker_profiles calls once more in a fresh process under `rocprofv3 --kernel-trace --stats` (a
run of its own: tracing slows the host) for the per-kernel split, k_score_profile_scan beside k_score_mean_scan.
"""

import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import score_rate  # noqa: E402  pylint: disable=wrong-import-position
import speakers_rate  # noqa: E402  pylint: disable=wrong-import-position
from uisrnn_amd import _capi, synth, weights  # noqa: E402  pylint: disable=wrong-import-position

GOLDEN = os.path.join(_ROOT, 'tests', 'golden')
TRACED_DONE = 'traced leg done'
_TRACE = re.compile(r'device_ms ([\d.]+) call_ms ([\d.]+)')


def _summary(rows):
  wall, sched, dev = (float(np.median([row[i] for row in rows])) for i in range(3))
  return {'wall_ms': wall, 'schedule_ms': sched, 'device_ms': dev, 'wall_ms_min': float(min(row[0] for row in rows)),
          'wall_ms_max': float(max(row[0] for row in rows))}


def leg(params, n_utt, n_frames, steps, warmup, lib, profiles_only=False):
  dim = int(params['observation_dim'])
  seqs, _, labels, offsets = score_rate.batch(n_utt, n_frames, dim)
  ptr, frames = score_rate.pinned_frames(lib, seqs, dim)
  width = int(labels.max()) + 1
  dec = _capi.Decoder(params, 0)
  try:
    calls = {'speaker_profiles': lambda: dec.speaker_profiles(frames, offsets, labels, width)}
    if not profiles_only:
      calls['score_speakers'] = lambda: dec.score_speakers(frames, offsets, labels, width + 1)
      calls['score_labels'] = lambda: dec.score_labels(frames, offsets, labels)
    times = {name: [] for name in calls}
    for step in range(warmup + steps):
      for name, fn in calls.items():  # (alternating: all see the same clocks and neighbours)
        t = speakers_rate.timed(fn)
        if step >= warmup:
          times[name].append(t)
    if not profiles_only:
      got = dec.speaker_profiles(frames, offsets, labels, width)
      assert np.array_equal(got['scores'].view(np.uint32), dec.score_labels(frames, offsets, labels).view(np.uint32))
      assert int(got['stats'][:, :, 0].sum()) == int(offsets[-1])
  finally:
    dec.close()
    lib.uis_host_free(ptr)
  out = {'utterances': n_utt, 'frames_per_utterance': n_frames, 'frames': int(offsets[-1]), 'width': width,
         'profile_bytes': n_utt * width * (16 + 3 * dim * 4)}
  for name, rows in times.items():
    out[name] = _summary(rows)
  if not profiles_only:
    for other in ('score_speakers', 'score_labels'):
      out['wall_ratio_to_' + other] = out['speaker_profiles']['wall_ms'] / out[other]['wall_ms']
      out['device_ratio_to_' + other] = out['speaker_profiles']['device_ms'] / out[other]['device_ms']
  return out


def session_leg(params, steps, warmup, slots=64, beam=10, pushed=40):
  dim = int(params['observation_dim'])
  seqs, _ = synth.make_utterances(6100, slots, pushed, dim)
  dec = _capi.Decoder(params, 0)
  dec.stream_begin(slots, beam, 64)
  os.environ['UIS_PROFILES_TRACE'] = os.environ['UIS_BINDINGS_TRACE'] = '1'
  try:
    dec.stream_push(seqs)
    calls = {'session_profiles': dec.stream_profiles, 'stream_bindings': dec.stream_bindings}
    times = {name: [] for name in calls}
    for step in range(warmup + steps):
      for name, fn in calls.items():
        box = {}

        def run(fn=fn, box=box):
          t0 = time.perf_counter()
          fn()
          box['wall'] = 1e3 * (time.perf_counter() - t0)
        m = _TRACE.search(score_rate.capture_stderr(run))
        if step >= warmup:
          times[name].append((box['wall'], float(m.group(1))))
    clusters = dec.stream_profiles()['n_clusters']
  finally:
    del os.environ['UIS_PROFILES_TRACE'], os.environ['UIS_BINDINGS_TRACE']
    dec.stream_end()
    dec.close()
  out = {'slots': slots, 'beam': beam, 'frames_per_slot': pushed, 'max_clusters': 16, 'clusters_mean': float(clusters.mean())}
  for name, rows in times.items():
    out[name] = {'wall_us': 1e3 * float(np.median([r[0] for r in rows])), 'device_us': 1e3 * float(np.median([r[1] for r in rows]))}
  return out


def traced(steps):
  """The 64 x 500 uis_speaker_profiles calls in a fresh process under rocprofv3: ({kernel: statistics}, exit status)."""
  tmp = tempfile.mkdtemp(prefix='profiles_rate_')
  try:
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', tmp, '-o', 'profiles', '--output-format', 'csv', '--',
           sys.executable, os.path.abspath(__file__), '--traced-leg', '--steps', str(steps)]
    with open(os.path.join(tmp, 'traced.err'), 'wb') as err, open(os.path.join(tmp, 'traced.out'), 'wb') as std:
      done = subprocess.run(cmd, check=False, stdout=std, stderr=err, timeout=300, cwd=tmp)
    with open(os.path.join(tmp, 'traced.out'), 'rb') as std:
      completed = TRACED_DONE.encode() in std.read()
    out = {}
    for path in glob.glob(os.path.join(tmp, '**', '*kernel_stats.csv'), recursive=True):
      with open(path) as f:
        for row in csv.DictReader(f):
          m = re.search(r'\b(k_\w+)(?:<[^(]*>)?\(', row['Name'])
          name = m.group(1) if m else row['Name']
          cell = out.setdefault(name, {'calls': 0, 'total_ns': 0.0})
          cell['calls'] += int(row['Calls'])
          cell['total_ns'] += float(row['TotalDurationNs'])
    if not completed or 'k_score_profile_scan' not in out:
      with open(os.path.join(tmp, 'traced.err'), 'rb') as err:
        tail = err.read()[-2000:].decode('utf-8', 'replace')
      raise RuntimeError('the rocprofv3 run (exit status {}, traced leg {}) left no usable statistics:\n{}'.format(
          done.returncode, 'completed' if completed else 'did NOT complete', tail))
    return out, done.returncode
  finally:
    shutil.rmtree(tmp, ignore_errors=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--steps', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--out', default=os.path.join(_ROOT, 'profiles', 'profiles_rate.json'))
  ap.add_argument('--traced-leg', action='store_true', help='(internal) the calls only, for the rocprofv3 run')
  a = ap.parse_args()
  os.environ['UIS_SCORE_TIMING'] = '1'
  lib = _capi.load_library()
  p256 = weights.load_checkpoint(os.path.join(GOLDEN, 'trained_d256.uisrnn'))
  if a.traced_leg:
    leg(p256, 64, 500, a.steps, 1, lib, profiles_only=True)
    print(TRACED_DONE, flush=True)  # (the handle is closed, the pinned buffer is freed: nothing of the library runs after this)
    return
  res = {'model': 'trained_d256'}
  res['64x500'] = leg(p256, 64, 500, a.steps, a.warmup, lib)
  print(json.dumps(res['64x500']), flush=True)
  res['1024x1000'] = leg(p256, 1024, 1000, max(a.steps // 2, 3), 1, lib)
  print(json.dumps(res['1024x1000']), flush=True)
  res['session_64_slots'] = session_leg(p256, 2 * a.steps, a.warmup)
  print(json.dumps(res['session_64_slots']), flush=True)
  traced_steps = min(a.steps, 5)
  kernels, status = traced(traced_steps)  # (the profiled run last: nothing else follows it)
  calls = traced_steps + 1
  res['kernels_64x500'] = {name: {'launches_per_call': cell['calls'] / calls, 'us_per_call': cell['total_ns'] / calls * 1e-3}
                           for name, cell in sorted(kernels.items(), key=lambda kv: -kv[1]['total_ns'])}
  res['traced_exit_status'] = status
  print(json.dumps(res['kernels_64x500']), flush=True)
  os.makedirs(os.path.dirname(a.out), exist_ok=True)
  with open(a.out, 'w') as f:
    json.dump(res, f, indent=1)
  print('wrote', a.out)


if __name__ == '__main__':
  main()
