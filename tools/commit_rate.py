"""What session commits cost on the MI355X.

  python tools/commit_rate.py call      [--steps 10] [--out profiles/commit_rate.json]
  python tools/commit_rate.py sustained [--frames 1000] [--out ...]
  python tools/commit_rate.py nbest | baseline      (the yardsticks alone: they also run on a build without
                                                     uis_stream_commit, UIS_LIB_PATH=<that library>)

trained_d256, synthetic utterances (uisrnn_amd.synth, seeds 7000..), beam 10.
  call       64 utterances x 500 frames in the window.  Wall time of one blocking uis_stream_commit (no horizon) and
             its device time (UIS_COMMIT_TRACE=1: the events around readout + prune + move), against the wall time of
             uis_stream_nbest(1) on the same session state.  The state is rebuilt for every commit (a commit moves it).
  sustained  an endless session: window 64, horizon 32, one frame per push, a commit when the window is full, for
             ordinary and persistent sessions, against the same pushes into a session whose max_frames holds everything.
             Reported: pushes per second either way, and what a commit costs (the call, and for a persistent
             session the push after it, which starts a new launch).
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

TRACE = re.compile(r'uis_stream_commit: utterances (\d+) window_frames (\d+) committed (\d+) prior_table_entries (\d+) '
                   r'device_ms ([\d.]+) call_ms ([\d.]+)')
BEAM = 10


def _frames(n_utt, n_frames, dim):
  return np.stack([synth.make_utterance(7000 + u, n_frames, dim)[0] for u in range(n_utt)]).astype(np.float32)


def _fill(dec, x, chunk=50):
  for lo in range(0, x.shape[1], chunk):
    dec.stream_push(x[:, lo:lo + chunk])


def _nbest1(dec, n_utt, total):
  labels = np.empty(max(total, 1), dtype=np.int32)
  stable = np.zeros(n_utt, dtype=np.int64)
  i32p = ctypes.POINTER(ctypes.c_int32)
  t0 = time.perf_counter()
  rc = dec._lib.uis_stream_nbest(dec._handle, 1, labels.ctypes.data_as(i32p), total, None, None,  # pylint: disable=protected-access
                                 stable.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
  ms = 1e3 * (time.perf_counter() - t0)
  assert rc == 0, rc
  return ms, stable


def leg_call(dec, a, with_commit):
  n_utt, n = 64, 500
  x = _frames(n_utt, n, dec.observation_dim)
  nbest_ms, commit_ms, device_ms, committed = [], [], [], 0
  for k in range(a.warmup + a.steps):
    dec.stream_begin(n_utt, BEAM, n)
    _fill(dec, x)
    per_state = [_nbest1(dec, n_utt, n_utt * n) for _ in range(5)]
    stable = per_state[-1][1]
    if with_commit:   # the bare C call, as the yardstick is timed
      box = {}
      labels = np.empty(n_utt * n, dtype=np.int32)
      counts = np.zeros(n_utt, dtype=np.int32)
      i32p = ctypes.POINTER(ctypes.c_int32)

      def run():
        t0 = time.perf_counter()
        box['rc'] = dec._lib.uis_stream_commit(dec._handle, None, labels.ctypes.data_as(i32p), labels.size,  # pylint: disable=protected-access
                                               counts.ctypes.data_as(i32p), None)
        box['ms'] = 1e3 * (time.perf_counter() - t0)
      m = TRACE.search(score_rate.capture_stderr(run))
      assert box['rc'] == 0 and counts.tolist() == [int(s) & ~1 for s in stable]
      committed = int(m.group(3))
    dec.stream_end()
    if k >= a.warmup:
      nbest_ms.append(float(np.median([ms for ms, _ in per_state[1:]])))
      if with_commit:
        commit_ms.append(box['ms'])
        device_ms.append(float(m.group(5)))
  res = {'utterances': n_utt, 'window_frames': n, 'beam': BEAM, 'steps': a.steps,
         'nbest1_wall_ms': float(np.median(nbest_ms)), 'stable_frames_mean': float(np.mean(stable))}
  if with_commit:
    res.update({'commit_wall_ms': float(np.median(commit_ms)), 'commit_device_ms': float(np.median(device_ms)),
                'committed_frames': committed, 'bp_bytes_in_window': n_utt * n * BEAM * 4,
                'wall_ratio': float(np.median(commit_ms)) / float(np.median(nbest_ms))})
  return res


def _run_pushes(dec, x, flags, window, horizon):
  """One frame per push; window None: max_frames holds everything, no commit."""
  n_utt, n = x.shape[0], x.shape[1]
  dec.stream_begin(n_utt, BEAM, n if window is None else window, flags=flags)
  hz = None if window is None else [horizon] * n_utt
  commit_s, after_s, commits, have, after = 0.0, 0.0, 0, 0, False
  t_begin = time.perf_counter()
  for t in range(n):
    if window is not None and have + 1 > window:
      t0 = time.perf_counter()
      dec.stream_commit(hz)
      commit_s += time.perf_counter() - t0
      commits += 1
      have = int(dec.stream_received().max())   # (the fullest window decides when the next commit is due)
      after = True
    t0 = time.perf_counter()
    dec.stream_push(x[:, t:t + 1])
    if after:
      after_s += time.perf_counter() - t0
      after = False
    have += 1
  total = time.perf_counter() - t_begin
  dec.stream_labels()
  dec.stream_end()
  return {'pushes_per_s': n / total, 'us_per_push': 1e6 * total / n, 'commits': commits,
          'us_per_commit_call': 1e6 * commit_s / max(commits, 1), 'us_push_after_commit': 1e6 * after_s / max(commits, 1)}


def leg_sustained(dec, a, with_commit):
  x = _frames(a.utterances, a.frames, dec.observation_dim)
  res = {'utterances': a.utterances, 'frames': a.frames, 'window': 64, 'horizon': 32, 'beam': BEAM}
  for name, flags in (('ordinary', 0), ('persistent', _capi.UIS_FLAG_PERSISTENT)):
    rows = {}
    for rep in range(a.reps):
      rows.setdefault('whole_stream_in_max_frames', []).append(_run_pushes(dec, x, flags, None, None))
      if with_commit:
        rows.setdefault('window_64_horizon_32', []).append(_run_pushes(dec, x, flags, 64, 32))
    best = {k: max(v, key=lambda r: r['pushes_per_s']) for k, v in rows.items()}
    if with_commit:
      best['overhead'] = best['whole_stream_in_max_frames']['pushes_per_s'] / best['window_64_horizon_32']['pushes_per_s'] - 1.0
    res[name] = best
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('leg', choices=['call', 'nbest', 'sustained', 'baseline'])
  ap.add_argument('--steps', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--frames', type=int, default=1000)
  ap.add_argument('--utterances', type=int, default=64)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--out', default=os.path.join(_ROOT, 'profiles', 'commit_rate.json'))
  a = ap.parse_args()
  os.environ['UIS_COMMIT_TRACE'] = '1'
  params = weights.load_checkpoint(os.path.join(score_rate.GOLDEN, 'trained_d256.uisrnn'))
  dec = _capi.Decoder(params, 0)
  try:
    if a.leg in ('call', 'nbest'):
      res = {a.leg: leg_call(dec, a, a.leg == 'call')}
    else:
      res = {a.leg: leg_sustained(dec, a, a.leg == 'sustained')}
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
