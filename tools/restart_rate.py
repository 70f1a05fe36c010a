"""What session restarts cost on the MI355X.

  python tools/restart_rate.py call    [--steps 10] [--out profiles/restart_rate.json]
  python tools/restart_rate.py service [--pushes 1000] [--every 10,100] [--out ...]

trained_d256, synthetic utterances (uisrnn_amd.synth, seeds 7000..), beam 10.
  call     64 utterances x 500 frames in the window.  Wall time of one blocking uis_stream_restart of 1 utterance and of
           all 64, and its device time (UIS_RESTART_TRACE=1: the events around readout + reset), against the wall time of
           uis_stream_labels on the same session state and against the only alternative a caller had before:
           uis_stream_end + uis_stream_begin of the same shape.  The state is rebuilt for every restart of all 64; a
           restart of one utterance takes the next slot each time.
  service  a persistent and an ordinary endless session of 64 slots: window 64, horizon 32, one frame per push, a commit
           when the window is full; one slot (round robin) is recycled every N pushes, against the same session with
           no restarts.  Reported: pushes per second, what a restart call costs and what the push after it costs (in
           a persistent session it starts a new resident launch).
Every leg merges its keys into --out.
"""

import argparse
import ctypes
import json
import os
import re
import sys
import time

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, 'tools'))

import score_rate  # noqa: E402  pylint: disable=wrong-import-position
from uisrnn_amd import _capi, synth, weights  # noqa: E402  pylint: disable=wrong-import-position

TRACE = re.compile(r'uis_stream_restart: utterances (\d+) selected (\d+) labels (\d+) device_ms ([\d.]+) call_ms ([\d.]+)')
BEAM = 10
_i32p = ctypes.POINTER(ctypes.c_int32)


def _frames(n_utt, n_frames, dim):
  return np.stack([synth.make_utterance(7000 + u, n_frames, dim)[0] for u in range(n_utt)]).astype(np.float32)


def _fill(dec, x, chunk=50):
  for lo in range(0, x.shape[1], chunk):
    dec.stream_push(x[:, lo:lo + chunk])


def _restart(dec, which, labels, counts, scores):
  """One bare C call: (wall ms, device ms of the trace line, labels handed out)."""
  box = {}

  def run():
    t0 = time.perf_counter()
    box['rc'] = dec._lib.uis_stream_restart(dec._handle, which.ctypes.data_as(_i32p), labels.ctypes.data_as(_i32p), labels.size,  # pylint: disable=protected-access
                                            counts.ctypes.data_as(_i32p), scores.ctypes.data_as(_capi._fp), None)  # pylint: disable=protected-access
    box['ms'] = 1e3 * (time.perf_counter() - t0)
  m = TRACE.search(score_rate.capture_stderr(run))
  assert box['rc'] == 0, box['rc']
  dec._stream_have[which != 0] = 0  # pylint: disable=protected-access
  return box['ms'], float(m.group(4)), int(m.group(3))


def _median(v):
  return float(np.median(v))


def leg_call(dec, a):
  n_utt, n = 64, 500
  x = _frames(n_utt, n, dec.observation_dim)
  labels = np.empty(n_utt * n, dtype=np.int32)
  counts = np.zeros(n_utt, dtype=np.int32)
  scores = np.zeros(n_utt, dtype=np.float32)
  rows = {k: [] for k in ('labels_ms', 'one_ms', 'one_dev', 'all_ms', 'all_dev', 'end_begin_ms', 'end_ms', 'begin_ms')}
  for k in range(a.warmup + a.steps):
    dec.stream_begin(n_utt, BEAM, n)
    _fill(dec, x)
    lab = []
    for _ in range(5):
      t0 = time.perf_counter()
      dec.stream_labels()
      lab.append(1e3 * (time.perf_counter() - t0))
    which = np.zeros(n_utt, dtype=np.int32)
    which[k % n_utt] = 1
    one = _restart(dec, which, labels, counts, scores)
    assert one[2] == n and counts[k % n_utt] == n
    dec.stream_push([x[u, :n] if u == k % n_utt else None for u in range(n_utt)])   # (the slot is full again)
    every = _restart(dec, np.ones(n_utt, dtype=np.int32), labels, counts, scores)
    assert every[2] == n_utt * n and dec.stream_committed().sum() == 0
    # the alternative: close the session and open one of the same shape (the state is already empty: nothing else differs)
    t0 = time.perf_counter()
    dec.stream_end()
    t1 = time.perf_counter()
    dec.stream_begin(n_utt, BEAM, n)
    t2 = time.perf_counter()
    dec.stream_end()
    if k >= a.warmup:
      rows['labels_ms'].append(_median(lab[1:]))
      rows['one_ms'].append(one[0]); rows['one_dev'].append(one[1])
      rows['all_ms'].append(every[0]); rows['all_dev'].append(every[1])
      rows['end_ms'].append(1e3 * (t1 - t0)); rows['begin_ms'].append(1e3 * (t2 - t1)); rows['end_begin_ms'].append(1e3 * (t2 - t0))
  med = {k: _median(v) for k, v in rows.items()}
  return {'utterances': n_utt, 'window_frames': n, 'beam': BEAM, 'steps': a.steps,
          'stream_labels_wall_ms': med['labels_ms'],
          'restart_1_wall_ms': med['one_ms'], 'restart_1_device_ms': med['one_dev'],
          'restart_64_wall_ms': med['all_ms'], 'restart_64_device_ms': med['all_dev'],
          'stream_end_wall_ms': med['end_ms'], 'stream_begin_wall_ms': med['begin_ms'], 'end_plus_begin_wall_ms': med['end_begin_ms'],
          'end_plus_begin_over_restart_64': med['end_begin_ms'] / med['all_ms'],
          'end_plus_begin_over_restart_1': med['end_begin_ms'] / med['one_ms']}


def _run_service(dec, x, flags, every):
  """One frame per push through a window of 64 (horizon 32); every `every` pushes the next slot is restarted (0: never)."""
  n_utt, n = x.shape[0], x.shape[1]
  window, hz = 64, [32] * x.shape[0]
  dec.stream_begin(n_utt, BEAM, window, flags=flags)
  which = np.zeros(n_utt, dtype=bool)
  restart_s, after_s, restarts, slot, after = 0.0, 0.0, 0, 0, False
  t_begin = time.perf_counter()
  for t in range(n):
    if int(dec._stream_have.max()) + 1 > window:  # pylint: disable=protected-access
      dec.stream_commit(hz)
    t0 = time.perf_counter()
    dec.stream_push(x[:, t:t + 1])
    if after:
      after_s += time.perf_counter() - t0
      after = False
    if every and t % every == every - 1:
      which[:] = False
      which[slot] = True
      slot = (slot + 1) % n_utt
      t0 = time.perf_counter()
      dec.stream_restart(which)
      restart_s += time.perf_counter() - t0
      restarts += 1
      after = True
  total = time.perf_counter() - t_begin
  dec.stream_labels()
  dec.stream_end()
  return {'pushes_per_s': n / total, 'us_per_push': 1e6 * total / n, 'restarts': restarts,
          'us_per_restart_call': 1e6 * restart_s / max(restarts, 1), 'us_push_after_restart': 1e6 * after_s / max(restarts, 1)}


def leg_service(dec, a):
  x = _frames(a.utterances, a.pushes, dec.observation_dim)
  res = {'utterances': a.utterances, 'pushes': a.pushes, 'window': 64, 'horizon': 32, 'beam': BEAM}
  for name, flags in (('ordinary', 0), ('persistent', _capi.UIS_FLAG_PERSISTENT)):
    rows = {}
    for _ in range(a.reps):
      for every in [0] + a.every:
        rows.setdefault('no_restarts' if not every else 'one_slot_every_{}_pushes'.format(every), []).append(
            _run_service(dec, x, flags, every))
    best = {k: max(v, key=lambda r: r['pushes_per_s']) for k, v in rows.items()}
    for k in list(best):
      if k != 'no_restarts':
        best[k]['slowdown'] = best['no_restarts']['pushes_per_s'] / best[k]['pushes_per_s'] - 1.0
    res[name] = best
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('leg', choices=['call', 'service'])
  ap.add_argument('--steps', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--pushes', type=int, default=1000)
  ap.add_argument('--utterances', type=int, default=64)
  ap.add_argument('--every', type=lambda s: [int(v) for v in s.split(',')], default=[10, 100])
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--out', default=os.path.join(_ROOT, 'profiles', 'restart_rate.json'))
  a = ap.parse_args()
  os.environ['UIS_RESTART_TRACE'] = '1' if a.leg == 'call' else '0'
  params = weights.load_checkpoint(os.path.join(score_rate.GOLDEN, 'trained_d256.uisrnn'))
  dec = _capi.Decoder(params, 0)
  try:
    res = {a.leg: leg_call(dec, a) if a.leg == 'call' else leg_service(dec, a)}
  finally:
    dec.close()
  res[a.leg]['library'] = os.environ.get('UIS_LIB_PATH', 'in-tree')
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
