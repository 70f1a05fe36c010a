"""What speaker retirement costs on the MI355X.

  python tools/retire_rate.py call      [--steps 5] [--out profiles/retire_rate.json]
  python tools/retire_rate.py sustained [--frames 1000] [--out ...]

trained_d256, synthetic utterances (uisrnn_amd.synth), beam 10, max_clusters 16.
  call       64 utterances x 500 frames in the window, behind 500 committed frames of other speakers (seeds 8000..;
             the window's are 7000..), so that every utterance has clusters to retire (and the commit behind them has
             sized the session's pinned landing block: the timed commit allocates nothing).  Wall and device time
             (UIS_RETIRE_TRACE=1: the events around scan + apply) of a query and of a retirement of everything
             retirable, and beside them uis_stream_commit (no horizon) on the same state, the yardstick of the
             earlier session features (UIS_COMMIT_TRACE=1).  The state is rebuilt for every timed retirement and commit.
  sustained  an endless 64-slot service over streams that walk through 30 speakers each: window 64, horizon 32, one
             frame per push.  Pushes per second of model.online(..., retire_at=12) against the same service without
             retire_at, how many utterances of each have hit the cluster cap at the end, and the push at which a
             service stops (without retire_at an utterance at the cap commits nothing any more: its window fills).
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
import uisrnn_amd  # noqa: E402  pylint: disable=wrong-import-position
from uisrnn_amd import _capi, synth, weights  # noqa: E402  pylint: disable=wrong-import-position

RETIRE = re.compile(r'uis_stream_retire: utterances (\d+) window_frames (\d+) selected (-?\d+) retired (\d+) '
                    r'device_ms ([\d.]+) call_ms ([\d.]+)')
COMMIT = re.compile(r'uis_stream_commit: .* device_ms ([\d.]+) call_ms ([\d.]+)')
BEAM, CAP = 10, 16
_i32p = ctypes.POINTER(ctypes.c_int32)


def _state(dec, old, new):
  """A session with new.shape[1] frames in the window behind a committed stretch of other speakers."""
  n_utt = new.shape[0]
  dec.stream_begin(n_utt, BEAM, new.shape[1] + old.shape[1], max_clusters=CAP)
  for lo in range(0, old.shape[1], 50):
    dec.stream_push(old[:, lo:lo + 50])
  dec.stream_commit([0] * n_utt)
  for lo in range(0, new.shape[1], 50):
    dec.stream_push(new[:, lo:lo + 50])


def _retire(dec, n_utt, everything):
  """One bare uis_stream_retire: (wall ms, device ms, retired, K, retirable counts)."""
  retired = np.zeros(n_utt * CAP, dtype=np.int32)
  able = np.zeros(n_utt * CAP, dtype=np.int32)
  counts, k_out, n_able = (np.zeros(n_utt, dtype=np.int32) for _ in range(3))
  offsets = np.zeros(n_utt + 1, dtype=np.int64)
  box = {}

  def run():
    t0 = time.perf_counter()
    box['rc'] = dec._lib.uis_stream_retire(  # pylint: disable=protected-access
        dec._handle, None, None if everything else offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), None,  # pylint: disable=protected-access
        retired.ctypes.data_as(_i32p), counts.ctypes.data_as(_i32p), k_out.ctypes.data_as(_i32p), able.ctypes.data_as(_i32p),
        n_able.ctypes.data_as(_i32p))
    box['ms'] = 1e3 * (time.perf_counter() - t0)
  m = RETIRE.search(score_rate.capture_stderr(run))
  assert box['rc'] == 0, box['rc']
  return box['ms'], float(m.group(5)), int(counts.sum()), k_out.copy(), int(n_able.sum())


def leg_call(dec, a):
  n_utt, n, behind = 64, 500, 500
  dim = dec.observation_dim
  new = np.stack([synth.make_utterance(7000 + u, n, dim)[0] for u in range(n_utt)]).astype(np.float32)
  old = np.stack([synth.make_utterance(8000 + u, behind, dim)[0] for u in range(n_utt)]).astype(np.float32)
  rows = {k: [] for k in ('query_wall_ms', 'query_device_ms', 'retire_wall_ms', 'retire_device_ms', 'commit_wall_ms',
                          'commit_device_ms')}
  info = {}
  for k in range(a.warmup + a.steps):
    _state(dec, old, new)
    queries = [_retire(dec, n_utt, False) for _ in range(5)]
    wall, dev, retired, k_after, _ = _retire(dec, n_utt, True)
    _, _, overflow, _ = dec.stream_labels()
    info = {'retirable': queries[-1][4], 'retired': retired, 'largest_K_before': int(queries[-1][3].max()),
            'largest_K_after': int(k_after.max()), 'utterances_at_the_cap': int((overflow != 0).sum())}
    assert retired == info['retirable']
    dec.stream_end()
    _state(dec, old, new)
    labels = np.empty(n_utt * n, dtype=np.int32)
    counts = np.zeros(n_utt, dtype=np.int32)
    box = {}

    def run():
      t0 = time.perf_counter()
      box['rc'] = dec._lib.uis_stream_commit(dec._handle, None, labels.ctypes.data_as(_i32p), labels.size,  # pylint: disable=protected-access
                                             counts.ctypes.data_as(_i32p), None)
      box['ms'] = 1e3 * (time.perf_counter() - t0)
    m = COMMIT.search(score_rate.capture_stderr(run))
    assert box['rc'] == 0
    dec.stream_end()
    if k >= a.warmup:
      rows['query_wall_ms'].append(float(np.median([q[0] for q in queries[1:]])))
      rows['query_device_ms'].append(float(np.median([q[1] for q in queries[1:]])))
      rows['retire_wall_ms'].append(wall)
      rows['retire_device_ms'].append(dev)
      rows['commit_wall_ms'].append(box['ms'])
      rows['commit_device_ms'].append(float(m.group(1)))
  res = {'utterances': n_utt, 'window_frames': n, 'committed_behind': behind, 'beam': BEAM, 'max_clusters': CAP, 'steps': a.steps}
  res.update({k: float(np.median(v)) for k, v in rows.items()})
  res.update(info)
  return res


def _service(model, args, x, retire_at):
  n_utt, n = x.shape[0], x.shape[1]
  kwargs = {} if retire_at is None else {'retire_at': retire_at}
  with model.online(n_utt, args, 64, horizon=32, **kwargs) as session:
    t0 = time.perf_counter()
    stopped = None
    pushed = 0
    try:
      for t in range(n):
        session.push(x[:, t:t + 1])
        pushed += 1
    except (RuntimeError, ValueError) as err:
      # with retire_at: the speakers inside the window alone do not fit.  Without it: an utterance at the cluster
      # cap commits nothing any more, its window fills up and the session refuses the push.  Reported, not hidden.
      stopped = str(err)
    total = time.perf_counter() - t0
    n = max(pushed, 1)
    _, _, overflow, _ = session._decoder.stream_labels()  # pylint: disable=protected-access
    gone = sum(len(g) for g in session._gone) if session._gone else 0  # pylint: disable=protected-access
  return {'pushes_per_s': n / total, 'us_per_push': 1e6 * total / n, 'pushes': pushed, 'stopped_by': stopped,
          'utterances_at_the_cap': int((overflow != 0).sum()), 'clusters_retired': gone}


def leg_sustained(params, a):
  dim = int(params['observation_dim'])
  model_args, _, args = uisrnn_amd.parse_arguments(
      ['--observation_dim', str(dim), '--rnn_hidden_size', str(int(params['rnn_hidden_size']))])
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params)
  args.beam_size, args.look_ahead, args.test_iteration, args.max_clusters = BEAM, 1, 1, CAP
  res = {'utterances': a.utterances, 'frames': a.frames, 'window': 64, 'horizon': 32, 'beam': BEAM, 'max_clusters': CAP,
         'retire_at': 12, 'retire_to': 6}
  # thirty speakers: what the policy is for; two to four (uisrnn_amd.synth's default): both services live, nothing to retire
  for name, kwargs in (('thirty_speakers', {'num_speakers': 30, 'mean_segment': 10.0}), ('few_speakers', {})):
    x = np.stack([synth.make_utterance(7000 + u, a.frames, dim, **kwargs)[0] for u in range(a.utterances)])
    rows = {'without_retire_at': [], 'with_retire_at': []}
    for _ in range(a.reps):
      rows['without_retire_at'].append(_service(model, args, x, None))
      rows['with_retire_at'].append(_service(model, args, x, 12))
    leg = {k: max(v, key=lambda r: r['pushes_per_s']) for k, v in rows.items()}
    leg['overhead'] = leg['without_retire_at']['pushes_per_s'] / leg['with_retire_at']['pushes_per_s'] - 1.0
    res[name] = leg
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('leg', choices=['call', 'sustained'])
  ap.add_argument('--steps', type=int, default=5)
  ap.add_argument('--warmup', type=int, default=1)
  ap.add_argument('--frames', type=int, default=1000)
  ap.add_argument('--utterances', type=int, default=64)
  ap.add_argument('--reps', type=int, default=2)
  ap.add_argument('--out', default=os.path.join(_ROOT, 'profiles', 'retire_rate.json'))
  a = ap.parse_args()
  os.environ['UIS_RETIRE_TRACE'] = '1'
  os.environ['UIS_COMMIT_TRACE'] = '1'
  params = weights.load_checkpoint(os.path.join(score_rate.GOLDEN, 'trained_d256.uisrnn'))
  if a.leg == 'call':
    dec = _capi.Decoder(params, 0)
    try:
      res = {'call': leg_call(dec, a)}
    finally:
      dec.close()
  else:
    os.environ.pop('UIS_RETIRE_TRACE')
    os.environ.pop('UIS_COMMIT_TRACE')
    res = {'sustained': leg_sustained(params, a)}
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
