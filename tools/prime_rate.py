"""Priming rate on the MI355X: uis_stream_prime against uis_score_labels on the same frames and labels.

  python tools/prime_rate.py [--steps 20] [--warmup 3] [--out profiles/prime_rate.json]

64 synthetic utterances (uisrnn_amd.synth, seeds 6000..) with 100-frame truth prefixes, trained_d256, the frames
in ONE pinned float32 buffer (uis_host_alloc) handed to both calls.  A session (beam 10, 64 utterances) is opened
for every priming call and closed after it, outside the timed region.  Reported: the median over `--steps` calls
of the wall time of the blocking call and of the device time (UIS_SCORE_TIMING=1: the library's own lines on
stderr -- the forced run's events, and for priming the commit kernels' on top), for both calls.  The yardstick
 is uis_score_labels: priming does that work plus one GRU row per chain and the copies.
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
from uisrnn_amd import _capi, weights  # noqa: E402  pylint: disable=wrong-import-position

FORCED = re.compile(r'chains (\d+) longest (\d+) schedule_ms ([\d.]+) device_ms ([\d.]+) total_ms ([\d.]+)')
COMMIT = re.compile(r'uis_stream_prime: utterances (\d+) chains (\d+) commit_device_ms ([\d.]+) call_ms ([\d.]+)')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--steps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--utterances', type=int, default=64)
  ap.add_argument('--frames', type=int, default=100)
  ap.add_argument('--out', default=os.path.join(_ROOT, 'profiles', 'prime_rate.json'))
  a = ap.parse_args()
  os.environ['UIS_SCORE_TIMING'] = '1'
  lib = _capi.load_library()
  params = weights.load_checkpoint(os.path.join(score_rate.GOLDEN, 'trained_d256.uisrnn'))
  dim = int(params['observation_dim'])
  seqs, _, labels, offsets = score_rate.batch(a.utterances, a.frames, dim)
  ptr, frames = score_rate.pinned_frames(lib, seqs, dim)
  dec = _capi.Decoder(params, 0)
  i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
  scores = np.zeros(a.utterances, dtype=np.float32)
  res = {'utterances': a.utterances, 'frames_per_utterance': a.frames, 'frames': int(offsets[-1]), 'steps': a.steps}
  try:
    def score():
      return lib.uis_score_labels(dec._handle, _capi._ptr(frames), offsets.ctypes.data_as(i64p), a.utterances,  # pylint: disable=protected-access
                                  labels.ctypes.data_as(i32p), _capi._ptr(scores), None)  # pylint: disable=protected-access

    def prime():
      return lib.uis_stream_prime(dec._handle, _capi._ptr(frames), offsets.ctypes.data_as(i64p),  # pylint: disable=protected-access
                                  labels.ctypes.data_as(i32p), _capi._ptr(scores))  # pylint: disable=protected-access

    def timed(call, session):
      wall, dev, commit = [], [], []
      for k in range(a.warmup + a.steps):
        if session:
          dec.stream_begin(a.utterances, 10, a.frames + 16)
        box = {}

        def run():
          t0 = time.perf_counter()
          box['rc'] = call()
          box['ms'] = 1e3 * (time.perf_counter() - t0)
        text = score_rate.capture_stderr(run)
        if session:
          dec.stream_end()
        assert box['rc'] == 0, (box['rc'], _capi.last_error(lib))
        m, c = FORCED.search(text), COMMIT.search(text)
        if k >= a.warmup:
          wall.append(box['ms'])
          dev.append(float(m.group(4)) + (float(c.group(3)) if c else 0.0))
          commit.append(float(c.group(3)) if c else 0.0)
        chains = int(m.group(1))
      return {'wall_ms': float(np.median(wall)), 'device_ms': float(np.median(dev)),
              'commit_device_ms': float(np.median(commit)), 'chains': chains}

    res['score_labels'] = timed(score, False)
    want = scores.copy()
    res['stream_prime'] = timed(prime, True)
    assert np.array_equal(want.view(np.uint32), scores.view(np.uint32)), 'the prefix NLL is uis_score_labels\' score'
    res['device_ratio'] = res['stream_prime']['device_ms'] / res['score_labels']['device_ms']
    res['wall_ratio'] = res['stream_prime']['wall_ms'] / res['score_labels']['wall_ms']
  finally:
    dec.close()
    lib.uis_host_free(ptr)
  print(json.dumps(res), flush=True)
  os.makedirs(os.path.dirname(a.out), exist_ok=True)
  with open(a.out, 'w') as f:
    json.dump(res, f, indent=1)
  print('wrote', a.out)


if __name__ == '__main__':
  main()
