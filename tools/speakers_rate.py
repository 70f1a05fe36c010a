"""What the whole row costs on the MI355X: uis_score_speakers beside uis_score_labels on the same batch.

  python tools/speakers_rate.py [--steps 10] [--warmup 2] [--out profiles/speakers_rate.json]

Two batches of synthetic utterances (uisrnn_amd.synth, seeds 6000.., as tools/score_rate.py), trained_d256, truth
labels, frames in ONE pinned float32 buffer (uis_host_alloc) handed to both calls: 64 x 500 and 1024 x 1000 frames.
width = the batch's largest cluster count + 1.  The calls alternate inside one process (uis_score_speakers twice: its rows
into a new pageable array, as Decoder.score_speakers returns them, and into a pinned one); per call the median wall
time of `--steps` blocking calls after `--warmup`, and the median of the library's own device time (UIS_SCORE_TIMING=1:
its line on stderr, events around the kernels, copies excluded).  The yardstick is uis_score_labels; DESIGN.md
section 23 expects the whole call within 1.25x of it.

Then the 64 x 500 uis_score_speakers calls once more in a fresh process under `rocprofv3 --kernel-trace --stats` (a run
of its own: tracing slows the host) for the per-kernel split.
"""

import argparse
import csv
import ctypes
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
from uisrnn_amd import _capi, weights  # noqa: E402  pylint: disable=wrong-import-position

GOLDEN = os.path.join(_ROOT, 'tests', 'golden')
TRACED_DONE = 'traced leg done'
_LINE = re.compile(r'schedule_ms ([\d.]+) device_ms ([\d.]+) total_ms ([\d.]+)')


def timed(fn):
  """(wall ms, the library's schedule / device ms) of one blocking call."""
  box = {}

  def run():
    t0 = time.perf_counter()
    fn()
    box['wall'] = 1e3 * (time.perf_counter() - t0)
  m = _LINE.search(score_rate.capture_stderr(run))
  return box['wall'], float(m.group(1)), float(m.group(2))


def leg(params, n_utt, n_frames, steps, warmup, lib, speakers_only=False):
  dim = int(params['observation_dim'])
  seqs, _, labels, offsets = score_rate.batch(n_utt, n_frames, dim)
  ptr, frames = score_rate.pinned_frames(lib, seqs, dim)
  width = int(labels.max()) + 2
  rows_ptr = ctypes.c_void_p()
  assert lib.uis_host_alloc(int(offsets[-1]) * width * 4, ctypes.byref(rows_ptr)) == 0
  pinned_rows = np.ctypeslib.as_array(ctypes.cast(rows_ptr, ctypes.POINTER(ctypes.c_float)), shape=(int(offsets[-1]), width))
  dec = _capi.Decoder(params, 0)
  try:
    calls = {'score_speakers': lambda: dec.score_speakers(frames, offsets, labels, width)}
    if not speakers_only:
      calls['score_speakers_pinned_rows'] = lambda: dec.score_speakers(frames, offsets, labels, width, losses_out=pinned_rows)
      calls['score_labels'] = lambda: dec.score_labels(frames, offsets, labels)
    times = {name: [] for name in calls}
    for step in range(warmup + steps):
      for name, fn in calls.items():  # (alternating: both see the same clocks and neighbours)
        t = timed(fn)
        if step >= warmup:
          times[name].append(t)
    if not speakers_only:
      scores, rows = dec.score_speakers(frames, offsets, labels, width)
      want, per = dec.score_labels(frames, offsets, labels, want_frame_losses=True)
      assert np.array_equal(scores.view(np.uint32), want.view(np.uint32))
      assert np.array_equal(rows[np.arange(labels.shape[0]), labels].view(np.uint32), per.view(np.uint32))
  finally:
    dec.close()
    lib.uis_host_free(ptr)
    lib.uis_host_free(rows_ptr)
  out = {'utterances': n_utt, 'frames_per_utterance': n_frames, 'frames': int(offsets[-1]), 'width': width,
         'rows_bytes': int(offsets[-1]) * width * 4}
  for name, t in times.items():
    wall, sched, dev = (float(np.median([row[i] for row in t])) for i in range(3))
    out[name] = {'wall_ms': wall, 'schedule_ms': sched, 'device_ms': dev,
                 'wall_ms_min': float(min(row[0] for row in t)), 'wall_ms_max': float(max(row[0] for row in t))}
  if not speakers_only:
    out['wall_ratio'] = out['score_speakers']['wall_ms'] / out['score_labels']['wall_ms']
    out['wall_ratio_pinned_rows'] = out['score_speakers_pinned_rows']['wall_ms'] / out['score_labels']['wall_ms']
    out['device_ratio'] = out['score_speakers']['device_ms'] / out['score_labels']['device_ms']
  return out


def traced(steps):
  """The 64 x 500 uis_score_speakers calls in a fresh process under rocprofv3: ({kernel: statistics}, exit status)."""
  tmp = tempfile.mkdtemp(prefix='speakers_rate_')
  try:
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', tmp, '-o', 'speakers', '--output-format', 'csv', '--',
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
    if not completed or 'k_score_speakers' not in out:
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
  ap.add_argument('--out', default=os.path.join(_ROOT, 'profiles', 'speakers_rate.json'))
  ap.add_argument('--traced-leg', action='store_true', help='(internal) the calls only, for the rocprofv3 run')
  a = ap.parse_args()
  os.environ['UIS_SCORE_TIMING'] = '1'
  lib = _capi.load_library()
  p256 = weights.load_checkpoint(os.path.join(GOLDEN, 'trained_d256.uisrnn'))
  if a.traced_leg:
    leg(p256, 64, 500, a.steps, 1, lib, speakers_only=True)
    print(TRACED_DONE, flush=True)  # (the handle is closed, the pinned buffer is freed: nothing of the library runs after this)
    return
  res = {'model': 'trained_d256'}
  res['64x500'] = leg(p256, 64, 500, a.steps, a.warmup, lib)
  print(json.dumps(res['64x500']), flush=True)
  res['1024x1000'] = leg(p256, 1024, 1000, max(a.steps // 2, 3), 1, lib)
  print(json.dumps(res['1024x1000']), flush=True)
  res['within_1.25x'] = bool(res['64x500']['wall_ratio'] <= 1.25 and res['1024x1000']['wall_ratio'] <= 1.25)
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
