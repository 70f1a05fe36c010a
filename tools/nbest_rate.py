"""Cost of the n-best readout on the MI355X: uis_last_decode_nbest beside the decode it reads.

  python tools/nbest_rate.py [--steps 10] [--warmup 2] [--out profiles/nbest_rate.json]

64 x 500 synthetic utterances (uisrnn_amd.synth, seeds 6000..), trained_d256, beam 10, n_best 10,
test_iteration 2 (the decode's default arguments: 1000 decode steps, of which a row is the last 500),
through the C ABI with the frames and the hypotheses' labels in pinned buffers (uis_host_alloc).
Wall times are the median of `--steps` blocking calls after `--warmup`.  The device times of k_nbest
and of k_backtrace come from a run of their own: this script starts itself once more under
`rocprofv3 --kernel-trace --stats` (a fresh process, the traced leg only) and reads the kernel
statistics that run leaves.  The gate of DESIGN.md section 12: k_nbest <= n_best x k_backtrace, the
cost of n_best separate back-traces.
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

from uisrnn_amd import _capi, synth, weights  # noqa: E402  pylint: disable=wrong-import-position

GOLDEN = os.path.join(_ROOT, 'tests', 'golden')
N_UTT, N_FRAMES, BEAM, N_BEST, TAU = 64, 500, 10, 10, 2   # (test_iteration 2: the decode's default arguments, as bench.py)
TRACED_DONE = 'traced leg: every library call has returned'


def pinned(lib, count, ctype, dtype):
  ptr = ctypes.c_void_p()
  assert lib.uis_host_alloc(count * np.dtype(dtype).itemsize, ctypes.byref(ptr)) == 0
  return ptr, np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), shape=(count,))


def median_ms(fn, steps, warmup):
  for _ in range(warmup):
    fn()
  times = []
  for _ in range(steps):
    t0 = time.perf_counter()
    fn()
    times.append(1e3 * (time.perf_counter() - t0))
  return float(np.median(times))


def leg(steps, warmup):
  """The decode and the readout, `steps` times each; returns their median wall times."""
  lib = _capi.load_library()
  params = weights.load_checkpoint(os.path.join(GOLDEN, 'trained_d256.uisrnn'))
  dim = int(params['observation_dim'])
  seqs, _ = synth.make_utterances(6000, N_UTT, N_FRAMES, dim)
  total = N_UTT * N_FRAMES
  offsets = np.arange(N_UTT + 1, dtype=np.int64) * N_FRAMES
  f_ptr, frames = pinned(lib, total * dim, ctypes.c_float, np.float32)
  frames.reshape(total, dim)[...] = np.concatenate(seqs, axis=0)
  l_ptr, labels = pinned(lib, total, ctypes.c_int32, np.int32)
  n_ptr, hyps = pinned(lib, N_BEST * total, ctypes.c_int32, np.int32)
  scores = np.empty(N_UTT * N_BEST, dtype=np.float32)
  counts = np.empty(N_UTT, dtype=np.int32)
  dec = _capi.Decoder(params, 0)
  i32p = ctypes.POINTER(ctypes.c_int32)

  def decode():
    out = dec.decode_host(f_ptr.value, offsets, BEAM, 1, TAU, l_ptr.value, None)
    assert out['status'] == 0

  def readout():
    rc = lib.uis_last_decode_nbest(dec._handle, N_BEST, ctypes.cast(n_ptr, i32p), N_BEST * total,
                                   scores.ctypes.data_as(_capi._fp), counts.ctypes.data_as(i32p))
    assert rc == 0, _capi.last_error(lib)

  try:
    decode_ms = median_ms(decode, steps, warmup)
    nbest_ms = median_ms(readout, steps, warmup)
    assert np.array_equal(hyps.reshape(N_UTT, N_BEST, N_FRAMES)[:, 0].reshape(-1), labels)
    live = int(counts.min())
  finally:
    dec.close()
    for p in (f_ptr, l_ptr, n_ptr):
      lib.uis_host_free(p)
  return {'utterances': N_UTT, 'frames_per_utterance': N_FRAMES, 'beam_size': BEAM, 'n_best': N_BEST,
          'test_iteration': TAU, 'decode_ms': decode_ms, 'nbest_ms': nbest_ms,
          'nbest_share_of_decode': nbest_ms / decode_ms, 'fewest_live_hypotheses': live}


def traced(steps):
  """The same calls in a fresh process under rocprofv3; returns ({kernel: statistics} of the two kernels, the
  traced process' exit status)."""
  tmp = tempfile.mkdtemp(prefix='nbest_rate_')
  try:
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', tmp, '-o', 'nbest', '--output-format', 'csv', '--',
           sys.executable, os.path.abspath(__file__), '--traced-leg', '--steps', str(steps)]
    with open(os.path.join(tmp, 'traced.err'), 'wb') as err, open(os.path.join(tmp, 'traced.out'), 'wb') as std:
      done = subprocess.run(cmd, check=False, stdout=std, stderr=err, timeout=300, cwd=tmp)
    with open(os.path.join(tmp, 'traced.out'), 'rb') as std:
      completed = TRACED_DONE.encode() in std.read()
    out = {}
    for path in glob.glob(os.path.join(tmp, '**', '*kernel_stats.csv'), recursive=True):
      with open(path) as f:
        for row in csv.DictReader(f):
          m = re.search(r'\b(k_nbest|k_backtrace)\(', row['Name'])  # (either may sit in an anonymous namespace)
          if m:
            out[m.group(1)] = {'calls': int(row['Calls']), 'mean_ns': float(row['AverageNs']),
                         'min_ns': float(row['MinNs']), 'max_ns': float(row['MaxNs'])}
    # The traced process may end with a signal although every call of the library has returned (seen: SIGSEGV
    # during interpreter exit under the profiler, after the statistics were written).  TRACED_DONE is printed
    # after the handle is closed and the pinned buffers are freed: with it the signal is the teardown's, without
    # it a call of the library did not come back and the numbers are not to be used.
    if not completed or 'k_nbest' not in out or 'k_backtrace' not in out:
      with open(os.path.join(tmp, 'traced.err'), 'rb') as err:
        tail = err.read()[-2000:].decode('utf-8', 'replace')
      raise RuntimeError('the rocprofv3 run (exit status {}, traced leg {}) left no usable statistics of k_nbest / '
                         'k_backtrace:\n{}'.format(done.returncode, 'completed' if completed else 'did NOT complete', tail))
    if done.returncode != 0:
      print('warning: the traced process exited with status {} AFTER its last library call returned '
            '(profiler / interpreter teardown); its kernel statistics were complete'.format(done.returncode), flush=True)
    return out, done.returncode
  finally:
    shutil.rmtree(tmp, ignore_errors=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--steps', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--out', default=os.path.join(_ROOT, 'profiles', 'nbest_rate.json'))
  ap.add_argument('--traced-leg', action='store_true', help='(internal) the calls only, for the rocprofv3 run')
  a = ap.parse_args()
  if a.traced_leg:
    leg(a.steps, 1)
    print(TRACED_DONE, flush=True)  # (the handle is closed, the pinned buffers are freed: nothing of the library runs after this)
    return
  res = leg(a.steps, a.warmup)
  print(json.dumps(res), flush=True)
  kernels, res['traced_exit_status'] = traced(a.steps)
  res['traced_leg_completed'] = True
  res['kernels'] = kernels
  if 'k_nbest' in kernels and 'k_backtrace' in kernels:
    res['k_nbest_over_k_backtrace'] = kernels['k_nbest']['mean_ns'] / kernels['k_backtrace']['mean_ns']
    res['gate_at_most_n_best_backtraces'] = res['k_nbest_over_k_backtrace'] <= N_BEST
  print(json.dumps(kernels), flush=True)
  os.makedirs(os.path.dirname(a.out), exist_ok=True)
  with open(a.out, 'w') as f:
    json.dump(res, f, indent=1)
  print('wrote', a.out)


if __name__ == '__main__':
  main()
