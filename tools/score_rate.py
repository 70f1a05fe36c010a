"""Scoring rate on the MI355X: uis_score_labels against uis_decode on the same batch.

  python tools/score_rate.py [--steps 10] [--warmup 2] [--out profiles/score_rate.json] [--quick]

Main line (the gate of DESIGN.md section 11): 64 x 500 synthetic utterances (uisrnn_amd.synth, seeds
6000..), trained_d256, truth labels, frames in ONE pinned float32 buffer (uis_host_alloc) handed to
both calls; the decode at the default arguments (beam 10, look_ahead 1, test_iteration 2).  Times are
the median wall time of `--steps` blocking calls after `--warmup`.  Also measured: the same through
the Python API (float64 lists: UISRNN.predict against UISRNN.score_labels), 1024 x 1000 frames, the
D 512 model (trained_d512), the host schedule's share of a call (UIS_SCORE_TIMING=1: the library's
own line on stderr) and the search-error table (how many utterances the model scores better under
their truth than under the decode, test_iteration 1, beam 1 / 10 / 50).

--quick: the main line only, fewer steps (for a rocprofv3 --kernel-trace --stats run).
"""

import argparse
import ctypes
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)

import uisrnn_amd  # noqa: E402  pylint: disable=wrong-import-position
from uisrnn_amd import _capi, synth, weights  # noqa: E402  pylint: disable=wrong-import-position

GOLDEN = os.path.join(_ROOT, 'tests', 'golden')


def first_appearance(ids):
  names = {}
  return np.array([names.setdefault(int(i), len(names)) for i in ids], dtype=np.int32)


def batch(n_utt, n_frames, dim, seed=6000):
  seqs, truth = synth.make_utterances(seed, n_utt, n_frames, dim)
  labels = np.concatenate([first_appearance(t) for t in truth])
  offsets = np.zeros(n_utt + 1, dtype=np.int64)
  offsets[1:] = np.cumsum([s.shape[0] for s in seqs])
  return seqs, truth, labels, offsets


def pinned_frames(lib, seqs, dim):
  total = sum(s.shape[0] for s in seqs)
  ptr = ctypes.c_void_p()
  assert lib.uis_host_alloc(total * dim * 4, ctypes.byref(ptr)) == 0
  arr = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_float)), shape=(total, dim))
  arr[...] = np.concatenate(seqs, axis=0)  # float64 -> float32 (RNE), as .float()
  return ptr, arr


def median_ms(fn, steps, warmup):
  for _ in range(warmup):
    fn()
  times = []
  for _ in range(steps):
    t0 = time.perf_counter()
    fn()
    times.append(1e3 * (time.perf_counter() - t0))
  return float(np.median(times))


def capture_stderr(fn):
  """fn() with file descriptor 2 sent to a temporary file; returns that text."""
  sys.stderr.flush()
  saved = os.dup(2)
  with tempfile.TemporaryFile(mode='w+b') as tmp:
    os.dup2(tmp.fileno(), 2)
    try:
      fn()
    finally:
      os.dup2(saved, 2)
      os.close(saved)
    tmp.seek(0)
    return tmp.read().decode('utf-8', 'replace')


def c_abi_leg(params, n_utt, n_frames, steps, warmup, lib):
  dim = int(params['observation_dim'])
  seqs, _, labels, offsets = batch(n_utt, n_frames, dim)
  ptr, frames = pinned_frames(lib, seqs, dim)
  dec = _capi.Decoder(params, 0)
  try:
    n = int(offsets[-1])
    score_ms = median_ms(lambda: dec.score_labels(frames, offsets, labels), steps, warmup)
    decode_ms = median_ms(lambda: dec.decode(frames, offsets, 10, 1, 2), steps, warmup)
    text = capture_stderr(lambda: dec.score_labels(frames, offsets, labels))
  finally:
    dec.close()
    lib.uis_host_free(ptr)
  out = {'utterances': n_utt, 'frames_per_utterance': n_frames, 'frames': n,
         'score_ms': score_ms, 'decode_ms': decode_ms,
         'score_frames_per_s': n / (score_ms * 1e-3), 'decode_frames_per_s': n / (decode_ms * 1e-3),
         'speedup': decode_ms / score_ms}
  m = re.search(r'chains (\d+) longest (\d+) schedule_ms ([\d.]+) device_ms ([\d.]+) total_ms ([\d.]+)', text)
  if m:
    out.update({'chains': int(m.group(1)), 'longest_chain': int(m.group(2)), 'schedule_ms': float(m.group(3)),
                'score_device_ms': float(m.group(4)), 'score_call_ms': float(m.group(5))})
  return out


def python_leg(steps, warmup):
  argv = ['--observation_dim', '256', '--rnn_hidden_size', '512']
  model_args, _, inference_args = uisrnn_amd.parse_arguments(argv)
  model = uisrnn_amd.UISRNN(model_args)
  model.load(os.path.join(GOLDEN, 'trained_d256.uisrnn'))
  seqs, truth, _, offsets = batch(64, 500, 256)
  ids = [t.tolist() for t in truth]
  n = int(offsets[-1])
  score_ms = median_ms(lambda: model.score_labels(seqs, ids), steps, warmup)
  predict_ms = median_ms(lambda: model.predict(seqs, inference_args), steps, warmup)
  return {'frames': n, 'score_ms': score_ms, 'predict_ms': predict_ms,
          'score_frames_per_s': n / (score_ms * 1e-3), 'predict_frames_per_s': n / (predict_ms * 1e-3),
          'speedup': predict_ms / score_ms}


def search_errors(params):
  """Utterances with NLL(truth) < NLL(decoded), test_iteration 1."""
  seqs, _, labels, offsets = batch(64, 500, 256)
  frames = np.concatenate(seqs).astype(np.float32)
  dec = _capi.Decoder(params, 0)
  truth_nll = dec.score_labels(frames, offsets, labels)
  out = {}
  for beam in (1, 10, 50):
    res = dec.decode(frames, offsets, beam, 1, 1)
    decoded_nll = dec.score_labels(frames, offsets, res['labels'])
    assert np.array_equal(decoded_nll.view(np.uint32), res['scores'].view(np.uint32))
    out['beam_{}'.format(beam)] = {
        'truth_better': int(np.sum(truth_nll < decoded_nll)),
        'labels_equal_truth': int(sum(np.array_equal(res['labels'][offsets[u]:offsets[u + 1]],
                                                     labels[offsets[u]:offsets[u + 1]]) for u in range(64)))}
  dec.close()
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--steps', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--out', default=os.path.join(_ROOT, 'profiles', 'score_rate.json'))
  ap.add_argument('--quick', action='store_true')
  a = ap.parse_args()
  os.environ['UIS_SCORE_TIMING'] = '1'
  lib = _capi.load_library()
  p256 = weights.load_checkpoint(os.path.join(GOLDEN, 'trained_d256.uisrnn'))
  res = {'main_64x500_d256': c_abi_leg(p256, 64, 500, a.steps if not a.quick else 3, a.warmup, lib)}
  print(json.dumps(res['main_64x500_d256']), flush=True)
  if a.quick:
    return
  res['gate_4x'] = res['main_64x500_d256']['speedup'] >= 4.0
  res['python_api_64x500_d256'] = python_leg(a.steps, a.warmup)
  print(json.dumps(res['python_api_64x500_d256']), flush=True)
  res['share_1024x1000_d256'] = c_abi_leg(p256, 1024, 1000, 3, 1, lib)
  print(json.dumps(res['share_1024x1000_d256']), flush=True)
  p512 = weights.load_checkpoint(os.path.join(GOLDEN, 'trained_d512.uisrnn'))
  res['d512_64x500'] = c_abi_leg(p512, 64, 500, a.steps, a.warmup, lib)
  print(json.dumps(res['d512_64x500']), flush=True)
  res['search_errors_64x500_d256_tau1'] = search_errors(p256)
  print(json.dumps(res['search_errors_64x500_d256_tau1']), flush=True)
  os.makedirs(os.path.dirname(a.out), exist_ok=True)
  with open(a.out, 'w') as f:
    json.dump(res, f, indent=1)
  print('wrote', a.out)


if __name__ == '__main__':
  main()
