"""Cost of the posterior readout on the MI355X: uis_last_decode_posterior beside the n-best readout of the same state.

  python tools/posterior_rate.py [--steps 30] [--warmup 5] [--out profiles/posterior_rate.json]

The n-best row's setup (tools/nbest_rate.py): 64 x 500 synthetic utterances (uisrnn_amd.synth, seeds 6000..),
trained_d256, test_iteration 2, through the C ABI with the frames and the per-frame results in pinned buffers
(uis_host_alloc); at beam 10 and at beam 256.  After ONE decode per beam the two readouts are called in turn on that
state -- posterior, n-best (n_best = beam_size), posterior, ... -- `--steps` times each after `--warmup`; reported are
the median wall time of a blocking call and its spread (min, quartiles, max).  The yardstick is the n-best readout:
the posterior call does the same walks and returns 2 floats per frame where the n-best returns beam_size ints.
The device times of k_posterior and k_nbest come from runs of their own: this script starts itself once per beam
under `rocprofv3 --kernel-trace --stats` (a fresh process, the calls only) and reads the kernel statistics.
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
N_UTT, N_FRAMES, TAU, BEAMS, TEMPERATURE = 64, 500, 2, (10, 256), 16.0
TRACED_DONE = 'traced leg: every library call has returned'


def pinned(lib, count, ctype, dtype):
  ptr = ctypes.c_void_p()
  assert lib.uis_host_alloc(count * np.dtype(dtype).itemsize, ctypes.byref(ptr)) == 0
  return ptr, np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), shape=(count,))


def spread(times):
  t = np.asarray(times)
  return {'median_ms': float(np.median(t)), 'min_ms': float(t.min()), 'q1_ms': float(np.percentile(t, 25)),
          'q3_ms': float(np.percentile(t, 75)), 'max_ms': float(t.max()), 'calls': int(t.size)}


def leg(beam, steps, warmup):
  """One decode at `beam`, then the two readouts in turn on its state."""
  lib = _capi.load_library()
  params = weights.load_checkpoint(os.path.join(GOLDEN, 'trained_d256.uisrnn'))
  dim = int(params['observation_dim'])
  seqs, _ = synth.make_utterances(6000, N_UTT, N_FRAMES, dim)
  total = N_UTT * N_FRAMES
  offsets = np.arange(N_UTT + 1, dtype=np.int64) * N_FRAMES
  f_ptr, frames = pinned(lib, total * dim, ctypes.c_float, np.float32)
  frames.reshape(total, dim)[...] = np.concatenate(seqs, axis=0)
  l_ptr, labels = pinned(lib, total, ctypes.c_int32, np.int32)
  n_ptr, hyps = pinned(lib, beam * total, ctypes.c_int32, np.int32)
  c_ptr, conf = pinned(lib, total, ctypes.c_float, np.float32)
  h_ptr, change = pinned(lib, total, ctypes.c_float, np.float32)
  scores = np.empty(N_UTT * beam, dtype=np.float32)
  weights_out = np.empty(N_UTT * beam, dtype=np.float32)
  counts = np.empty(N_UTT, dtype=np.int32)
  live = np.empty(N_UTT, dtype=np.int32)
  dec = _capi.Decoder(params, 0)
  i32p = ctypes.POINTER(ctypes.c_int32)

  def posterior():
    rc = lib.uis_last_decode_posterior(dec._handle, TEMPERATURE, ctypes.cast(c_ptr, _capi._fp), ctypes.cast(h_ptr, _capi._fp),
                                       total, weights_out.ctypes.data_as(_capi._fp), live.ctypes.data_as(i32p))
    assert rc == 0, _capi.last_error(lib)

  def nbest():
    rc = lib.uis_last_decode_nbest(dec._handle, beam, ctypes.cast(n_ptr, i32p), beam * total,
                                   scores.ctypes.data_as(_capi._fp), counts.ctypes.data_as(i32p))
    assert rc == 0, _capi.last_error(lib)

  try:
    t0 = time.perf_counter()
    out = dec.decode_host(f_ptr.value, offsets, beam, 1, TAU, l_ptr.value, None)
    decode_ms = 1e3 * (time.perf_counter() - t0)
    times = {'posterior': [], 'nbest': []}
    for k in range(warmup + steps):
      for name, fn in (('posterior', posterior), ('nbest', nbest)):
        t0 = time.perf_counter()
        fn()
        if k >= warmup:
          times[name].append(1e3 * (time.perf_counter() - t0))
    assert np.array_equal(hyps.reshape(N_UTT, beam, N_FRAMES)[:, 0].reshape(-1), labels)
    assert np.array_equal(live, counts)
    # the readout against its definition, on the host, for the first utterance
    rows, s = hyps.reshape(N_UTT, beam, N_FRAMES)[0, :live[0]], scores[:live[0]].astype(np.float64)
    w = np.exp(-(s - s[0]) / TEMPERATURE)
    w /= w.sum()
    err = float(np.abs((w[:, None] * (rows == rows[0])).sum(axis=0) - conf[:N_FRAMES]).max())
    assert err <= (int(live[0]) + 8) * 2.0 ** -23, err
    res = {'beam_size': beam, 'decode_status': int(out['status']), 'first_decode_ms': decode_ms,
           'fewest_live_hypotheses': int(live.min()), 'most_live_hypotheses': int(live.max()),
           'frames_with_confidence_below_0.999': int((conf < 0.999).sum()), 'frames': total,
           'posterior_call': spread(times['posterior']), 'nbest_call': spread(times['nbest'])}
    res['posterior_over_nbest_per_call'] = res['posterior_call']['median_ms'] / res['nbest_call']['median_ms']
  finally:
    dec.close()
    for p in (f_ptr, l_ptr, n_ptr, c_ptr, h_ptr):
      lib.uis_host_free(p)
  return res


def traced(beam, steps):
  """The same calls in a fresh process under rocprofv3; returns ({kernel: statistics}, the traced process' exit status)."""
  tmp = tempfile.mkdtemp(prefix='posterior_rate_')
  try:
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', tmp, '-o', 'posterior', '--output-format', 'csv', '--',
           sys.executable, os.path.abspath(__file__), '--traced-leg', str(beam), '--steps', str(steps)]
    with open(os.path.join(tmp, 'traced.err'), 'wb') as err, open(os.path.join(tmp, 'traced.out'), 'wb') as std:
      done = subprocess.run(cmd, check=False, stdout=std, stderr=err, timeout=300, cwd=tmp)
    with open(os.path.join(tmp, 'traced.out'), 'rb') as std:
      completed = TRACED_DONE.encode() in std.read()
    out = {}
    for path in glob.glob(os.path.join(tmp, '**', '*kernel_stats.csv'), recursive=True):
      with open(path) as f:
        for row in csv.DictReader(f):
          m = re.search(r'\b(k_posterior|k_nbest)\(', row['Name'])  # (either may sit in an anonymous namespace)
          if m:
            out[m.group(1)] = {'calls': int(row['Calls']), 'mean_ns': float(row['AverageNs']),
                               'min_ns': float(row['MinNs']), 'max_ns': float(row['MaxNs'])}
    # (as tools/nbest_rate.py: a signal during the profiler's teardown, after TRACED_DONE, does not spoil the statistics)
    if not completed or 'k_posterior' not in out or 'k_nbest' not in out:
      with open(os.path.join(tmp, 'traced.err'), 'rb') as err:
        tail = err.read()[-2000:].decode('utf-8', 'replace')
      raise RuntimeError('the rocprofv3 run (exit status {}, traced leg {}) left no usable statistics:\n{}'.format(
          done.returncode, 'completed' if completed else 'did NOT complete', tail))
    return out, done.returncode
  finally:
    shutil.rmtree(tmp, ignore_errors=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--steps', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--out', default=os.path.join(_ROOT, 'profiles', 'posterior_rate.json'))
  ap.add_argument('--traced-leg', type=int, default=0, metavar='BEAM', help='(internal) the calls only, for the rocprofv3 run')
  a = ap.parse_args()
  if a.traced_leg:
    leg(a.traced_leg, a.steps, 1)
    print(TRACED_DONE, flush=True)  # (the handle is closed, the pinned buffers are freed: nothing of the library runs after this)
    return
  res = {'utterances': N_UTT, 'frames_per_utterance': N_FRAMES, 'test_iteration': TAU, 'temperature': TEMPERATURE, 'beams': {}}
  for beam in BEAMS:
    res['beams'][str(beam)] = leg(beam, a.steps, a.warmup)
    print(json.dumps(res['beams'][str(beam)]), flush=True)
  for beam in BEAMS:   # (the profiled runs last: nothing else follows them)
    kernels, status = traced(beam, min(a.steps, 10))
    row = res['beams'][str(beam)]
    row['kernels'], row['traced_exit_status'] = kernels, status
    row['k_posterior_over_k_nbest'] = kernels['k_posterior']['mean_ns'] / kernels['k_nbest']['mean_ns']
    print(json.dumps(kernels), flush=True)
    if status != 0:
      print('the traced process exited with status {} after its last library call returned; stopping here'.format(status), flush=True)
      break
  os.makedirs(os.path.dirname(a.out), exist_ok=True)
  with open(a.out, 'w') as f:
    json.dump(res, f, indent=1)
  print('wrote', a.out)


if __name__ == '__main__':
  main()
