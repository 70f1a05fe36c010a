"""What moving a live utterance costs on the MI355X.

  python tools/migrate_rate.py call    [--steps 10] [--out profiles/migrate_rate.json]
  python tools/migrate_rate.py service [--pushes 1000] [--every 10] [--out ...]

trained_d256, synthetic utterances (uisrnn_amd.synth, seeds 7000..), beam 10.
  call     64 utterances x 500 frames in the window.  Wall time of one blocking uis_stream_export and of one
           uis_stream_import of 1 utterance (bare C calls), their device time (UIS_MIGRATE_TRACE=1: the events around
           pack + copy) and the blob's size, and beside them, in the same process and session state, the project's
           yardsticks: uis_stream_restart of that utterance (a bare C call; UIS_RESTART_TRACE=1) and uis_stream_prime
           of its window labels into the restarted slot (through _capi; UIS_SCORE_TIMING=1: the forced run's device
           time plus the commit's) -- what a caller had to do before to continue a stream elsewhere, and it keeps one
           hypothesis of the beam.  The utterance takes the next slot each step; export -> restart -> import puts it
           back, restart -> prime follows.
  service  an ordinary and a persistent endless session of 64 streams in 65 slots: window 64, horizon 32, one frame
           per push, a commit when the window is full; every N pushes one stream (round robin) moves into the free
           slot (export, import, restart of the slot it left), against the same session with no moves.  Reported:
           pushes per second, what a move costs and what the push after it costs.
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

MIGRATE = re.compile(r'uis_stream_(export|import): .* slots (\d+) bytes (\d+) .* device_ms ([\d.]+) call_ms ([\d.]+)')
RESTART = re.compile(r'uis_stream_restart: .* device_ms ([\d.]+) call_ms ([\d.]+)')
FORCED = re.compile(r'frames \d+ chains \d+ longest \d+ schedule_ms [\d.]+ device_ms ([\d.]+)')
PRIME = re.compile(r'uis_stream_prime: .* commit_device_ms ([\d.]+) call_ms ([\d.]+)')
BEAM = 10
_i32p = ctypes.POINTER(ctypes.c_int32)


def _frames(n_utt, n_frames, dim):
  return np.stack([synth.make_utterance(7000 + u, n_frames, dim)[0] for u in range(n_utt)]).astype(np.float32)


def _timed(fn):
  """(result, wall ms, what the call wrote to stderr)."""
  box = {}

  def run():
    t0 = time.perf_counter()
    box['out'] = fn()
    box['ms'] = 1e3 * (time.perf_counter() - t0)
  text = score_rate.capture_stderr(run)
  return box['out'], box['ms'], text


def _median(v):
  return float(np.median(v))


def leg_call(dec, a):
  n_utt, n = 64, 500
  x = _frames(n_utt, n, dec.observation_dim)
  lib, handle = dec._lib, dec._handle  # pylint: disable=protected-access
  dec.stream_begin(n_utt, BEAM, n)
  for lo in range(0, n, 50):
    dec.stream_push(x[:, lo:lo + 50])
  bound = dec.stream_export_bound()
  buf = ctypes.create_string_buffer(bound)
  size = ctypes.c_int64(0)
  out_labels, out_counts = np.empty(n, dtype=np.int32), np.zeros(n_utt, dtype=np.int32)
  keys = ('export_ms', 'export_dev', 'import_ms', 'import_dev', 'restart_ms', 'restart_dev', 'prime_ms', 'prime_dev', 'bytes', 'slots')
  rows = {k: [] for k in keys}
  for k in range(a.warmup + a.steps):
    u = k % n_utt
    window = dec.stream_labels()[0][u]
    which = [v == u for v in range(n_utt)]
    rc, ex_ms, text = _timed(lambda: lib.uis_stream_export(handle, u, buf, bound, ctypes.byref(size)))  # pylint: disable=cell-var-from-loop
    assert rc == 0, rc
    ex = MIGRATE.search(text)
    blob = ctypes.string_at(buf, size.value)
    sel = np.asarray(which, dtype=np.int32)
    rc, rs_ms, text = _timed(lambda: lib.uis_stream_restart(handle, sel.ctypes.data_as(_i32p), out_labels.ctypes.data_as(_i32p), n,  # pylint: disable=cell-var-from-loop
                                                             out_counts.ctypes.data_as(_i32p), None, None))
    assert rc == 0 and out_counts[u] == n, rc
    dec._stream_have[u] = 0  # pylint: disable=protected-access
    rs = RESTART.search(text)
    rc, im_ms, text = _timed(lambda: lib.uis_stream_import(handle, u, blob, len(blob)))  # pylint: disable=cell-var-from-loop
    assert rc == 0, rc
    im = MIGRATE.search(text)
    dec._stream_have[u] = n  # pylint: disable=protected-access
    assert np.array_equal(dec.stream_labels()[0][u], window)   # the utterance is back
    dec.stream_restart(which)
    chunks, labels = [None] * n_utt, [None] * n_utt
    chunks[u], labels[u] = x[u], np.asarray(score_rate.first_appearance(window), dtype=np.int32)
    _, pr_ms, text = _timed(lambda: dec.stream_prime(chunks, labels))  # pylint: disable=cell-var-from-loop
    pr, forced = PRIME.search(text), FORCED.search(text)
    if k >= a.warmup:
      rows['export_ms'].append(ex_ms); rows['export_dev'].append(float(ex.group(4)))
      rows['import_ms'].append(im_ms); rows['import_dev'].append(float(im.group(4)))
      rows['restart_ms'].append(rs_ms); rows['restart_dev'].append(float(rs.group(1)))
      rows['prime_ms'].append(pr_ms); rows['prime_dev'].append(float(pr.group(1)) + float(forced.group(1)))
      rows['bytes'].append(int(ex.group(3))); rows['slots'].append(int(ex.group(2)))
  dec.stream_end()
  med = {k: _median(v) for k, v in rows.items()}
  return {'utterances': n_utt, 'window_frames': n, 'beam': BEAM, 'steps': a.steps,
          'blob_bytes': med['bytes'], 'blob_slots': med['slots'], 'export_bound_bytes': bound,
          'export_1_wall_ms': med['export_ms'], 'export_1_device_ms': med['export_dev'],
          'import_1_wall_ms': med['import_ms'], 'import_1_device_ms': med['import_dev'],
          'restart_1_wall_ms': med['restart_ms'], 'restart_1_device_ms': med['restart_dev'],
          'prime_1_wall_ms': med['prime_ms'], 'prime_1_device_ms': med['prime_dev'],
          'prime_over_export_plus_import_wall': med['prime_ms'] / (med['export_ms'] + med['import_ms']),
          'prime_over_import_wall': med['prime_ms'] / med['import_ms']}


def _run_service(dec, x, flags, every):
  """One frame per push through a window of 64 (horizon 32), 64 streams in 65 slots; every `every` pushes the next
  stream moves into the free slot (0: never)."""
  n_streams, n = x.shape[0], x.shape[1]
  n_slots, window = n_streams + 1, 64
  hz = [32] * n_slots
  dec.stream_begin(n_slots, BEAM, window, flags=flags)
  slot_of, free = list(range(n_streams)), n_streams
  which = np.zeros(n_slots, dtype=bool)
  move_s, after_s, moves, nxt, after = 0.0, 0.0, 0, 0, False
  t_begin = time.perf_counter()
  for t in range(n):
    if int(dec._stream_have.max()) + 1 > window:  # pylint: disable=protected-access
      dec.stream_commit(hz)
    chunks = [None] * n_slots
    for s in range(n_streams):
      chunks[slot_of[s]] = x[s, t:t + 1]
    t0 = time.perf_counter()
    dec.stream_push(chunks)
    if after:
      after_s += time.perf_counter() - t0
      after = False
    if every and t % every == every - 1:
      t0 = time.perf_counter()
      dec.stream_import(free, dec.stream_export(slot_of[nxt]))
      which[:] = False
      which[slot_of[nxt]] = True
      dec.stream_restart(which)
      slot_of[nxt], free = free, slot_of[nxt]
      nxt = (nxt + 1) % n_streams
      move_s += time.perf_counter() - t0
      moves += 1
      after = True
  total = time.perf_counter() - t_begin
  dec.stream_labels()
  dec.stream_end()
  return {'pushes_per_s': n / total, 'us_per_push': 1e6 * total / n, 'moves': moves,
          'us_per_move': 1e6 * move_s / max(moves, 1), 'us_push_after_move': 1e6 * after_s / max(moves, 1)}


def leg_service(dec, a):
  x = _frames(a.utterances, a.pushes, dec.observation_dim)
  res = {'streams': a.utterances, 'slots': a.utterances + 1, 'pushes': a.pushes, 'window': 64, 'horizon': 32, 'beam': BEAM}
  for name, flags in (('ordinary', 0), ('persistent', _capi.UIS_FLAG_PERSISTENT)):
    rows = {}
    try:
      for _ in range(a.reps):
        for every in [0] + a.every:
          rows.setdefault('no_moves' if not every else 'one_stream_every_{}_pushes'.format(every), []).append(
              _run_service(dec, x, flags, every))
    except _capi.HipLibraryError as err:   # (UIS_FLAG_PERSISTENT does not take every shape)
      if err.status != _capi.UIS_ERR_UNSUPPORTED:
        raise
      res[name] = 'unsupported'
      continue
    best = {k: max(v, key=lambda r: r['pushes_per_s']) for k, v in rows.items()}
    for k in list(best):
      if k != 'no_moves':
        best[k]['slowdown'] = best['no_moves']['pushes_per_s'] / best[k]['pushes_per_s'] - 1.0
    res[name] = best
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('leg', choices=['call', 'service'])
  ap.add_argument('--steps', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--pushes', type=int, default=1000)
  ap.add_argument('--utterances', type=int, default=64)
  ap.add_argument('--every', type=lambda s: [int(v) for v in s.split(',')], default=[10])
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--out', default=os.path.join(_ROOT, 'profiles', 'migrate_rate.json'))
  a = ap.parse_args()
  for knob in ('UIS_MIGRATE_TRACE', 'UIS_RESTART_TRACE', 'UIS_SCORE_TIMING'):
    os.environ[knob] = '1' if a.leg == 'call' else '0'
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
