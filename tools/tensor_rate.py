"""What the device-tensor entry points cost and save on the MI355X.  Nothing here is a threshold
fixed in advance: the figures are recorded, losses included; the one condition is stated with its margin.

  python tools/tensor_rate.py --parent DIR [--runs 5] [--legs push,decode] [--out profiles/tensor_rate.json]

push    a 64-slot session on trained_d256, beam 10, synthetic utterances (uisrnn_amd.synth), one frame and 16 frames
        per push; the frames of every push START in a float32 device tensor [64, n, 256] (an encoder's output):
          push_tensors   OnlineSession's route now: Decoder.stream_push_tensors of the tensor's slice
          today          the only route before: .double().cpu().numpy(), then Decoder.stream_push
          host           Decoder.stream_push from a host numpy array (the frames never were on the device) -- this
                         commit and a built checkout of the parent commit (--parent): the two must overlap
decode  64 utterances x 500 frames x 256, beam 10, test_iteration 2, through UISRNN:
          predict_tensors at float64, float32 and float16 (a list of device tensors)
          today          the same device tensors: [t.double().cpu().numpy() ...], then predict
          predict        the float64 list already on the host
          decode_device  Decoder.decode_device on the packed float32 stream resident in HBM: the floor
Every run is a process of its own per group (this commit's push legs, the parent's, the decode legs), the groups
interleaved, --runs each; microseconds per push, milliseconds per decode, host clock around blocking calls.
The condition: a device-tensor leg is no slower than today's route from the same starting point (ranges compared).
"""

import argparse
import json
import os
import subprocess
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PUSH_WORKER = r'''
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import torch
from uisrnn_amd import _capi, synth, weights
frames, legs = int(sys.argv[1]), sys.argv[2].split(',')
U = 64
params = weights.load_checkpoint(os.path.join('tests', 'golden', 'trained_d256.uisrnn'))
dim = int(params['observation_dim'])
x = np.stack([synth.make_utterance(7000 + u, frames, dim)[0] for u in range(U)]).astype(np.float32)
x_dev = torch.from_numpy(x).cuda()
torch.cuda.synchronize()
res = {}
for per_push in (1, 16):
  for leg in legs:
    dec = _capi.Decoder(params)
    dec.stream_begin(U, 10, frames, max_clusters=16)
    try:
      def push(t):
        if leg == 'push_tensors':
          dec.stream_push_tensors(x_dev[:, t:t + per_push])
        elif leg == 'today':
          dec.stream_push(x_dev[:, t:t + per_push].double().cpu().numpy())
        else:
          dec.stream_push(x[:, t:t + per_push])
      push(0)   # (the first push: allocations, the cooperative launch's check)
      n = 0
      t0 = time.perf_counter()
      for t in range(per_push, frames - per_push + 1, per_push):
        push(t)
        n += 1
      res['%s_%d' % (leg, per_push)] = 1e6 * (time.perf_counter() - t0) / n
      res['labels_%s_%d' % (leg, per_push)] = int(np.concatenate(dec.stream_labels()[0]).astype(np.int64).sum())
    finally:
      dec.stream_end()
      dec.close()
print('RESULT ' + json.dumps(res), flush=True)
'''

_DECODE_WORKER = r'''
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import torch
import uisrnn_amd
from uisrnn_amd import _capi, synth, weights
U, N, reps = 64, 500, 3
params = weights.load_checkpoint(os.path.join('tests', 'golden', 'trained_d256.uisrnn'))
dim = int(params['observation_dim'])
model_args, _, args = uisrnn_amd.parse_arguments([])
model_args.observation_dim = dim
model = uisrnn_amd.UISRNN(model_args)
model.load_params(params)
args.beam_size, args.look_ahead, args.test_iteration = 10, 1, 2
seqs = [synth.make_utterance(9000 + u, N, dim)[0].astype(np.float64) for u in range(U)]
dev = {name: [torch.from_numpy(s).to(dt).cuda() for s in seqs]
       for name, dt in (('f64', torch.float64), ('f32', torch.float32), ('f16', torch.float16))}
packed = torch.from_numpy(np.concatenate(seqs).astype(np.float32)).cuda()
offsets = np.arange(U + 1, dtype=np.int64) * N
d_labels = torch.empty(U * N, dtype=torch.int32, device='cuda')
d_scores = torch.empty(U, dtype=torch.float32, device='cuda')
torch.cuda.synchronize()
dec = model._get_decoder()
legs = {
    'predict_tensors_f64': lambda: model.predict_tensors(dev['f64'], args),
    'predict_tensors_f32': lambda: model.predict_tensors(dev['f32'], args),
    'predict_tensors_f16': lambda: model.predict_tensors(dev['f16'], args),
    'today_f64': lambda: model.predict([t.double().cpu().numpy() for t in dev['f64']], args),
    'today_f32': lambda: model.predict([t.double().cpu().numpy() for t in dev['f32']], args),
    'today_f16': lambda: model.predict([t.double().cpu().numpy() for t in dev['f16']], args),
    'predict': lambda: model.predict(seqs, args),
    'decode_device': lambda: dec.decode_device(packed.data_ptr(), offsets, 10, 1, 2, d_labels.data_ptr(), d_scores.data_ptr()),
}
res = {}
for name, call in legs.items():
  call()   # (warm: workspaces, the control-word placement trials of a new shape)
  call()
for _ in range(reps):   # the legs interleaved
  for name, call in legs.items():
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    res.setdefault(name, []).append(1e3 * (time.perf_counter() - t0))
res = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
same = [a.tolist() for a in model.predict_tensors(dev['f64'], args)] == model.predict(seqs, args)
res['labels_equal_predict'] = bool(same)
print('RESULT ' + json.dumps(res), flush=True)
'''


def _median(values):
  values = sorted(values)
  return values[len(values) // 2] if values else None


def _run(tree, worker, *argv):
  done = subprocess.run([sys.executable, '-c', worker] + [str(a) for a in argv], cwd=tree, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, check=True, timeout=400)
  return json.loads([l for l in done.stdout.decode().splitlines() if l.startswith('RESULT ')][-1][7:])


def _against(new, old, what):
  """The condition, with its margin: ranges of the runs, and the ratio of the medians."""
  ratio = _median(new) / _median(old)
  if max(new) < min(old):
    verdict = 'faster: the ranges separate'
  elif min(new) > max(old):
    verdict = 'SLOWER: the ranges separate'
  else:
    verdict = 'the ranges overlap'
  return {'what': what, 'verdict': verdict, 'median_ratio': ratio, 'saved_percent': 100.0 * (1.0 - ratio)}


def _rows(runs):
  keys = sorted({k for r in runs for k in r})
  return {k: [r[k] for r in runs if k in r] for k in keys}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--parent', required=True, help='a built checkout of the parent commit')
  ap.add_argument('--runs', type=int, default=5)
  ap.add_argument('--frames', type=int, default=320)
  ap.add_argument('--legs', type=lambda v: v.split(','), default=['push', 'decode'])
  ap.add_argument('--out', default=os.path.join(_ROOT, 'profiles', 'tensor_rate.json'))
  a = ap.parse_args()
  a.parent = os.path.abspath(a.parent)
  if not os.path.exists(os.path.join(a.parent, 'uisrnn_amd', '_capi.py')):
    raise SystemExit('--parent: a checkout of the parent commit with its library built')
  this_push, parent_push, decode = [], [], []
  for run in range(a.runs):
    if 'push' in a.legs:
      this_push.append(_run(_ROOT, _PUSH_WORKER, a.frames, 'push_tensors,today,host'))
      parent_push.append(_run(a.parent, _PUSH_WORKER, a.frames, 'host'))
      print(run, this_push[-1], parent_push[-1], flush=True)
    if 'decode' in a.legs:
      decode.append(_run(_ROOT, _DECODE_WORKER))
      print(run, decode[-1], flush=True)
  res = {}
  if this_push:
    rows, parent = _rows(this_push), _rows(parent_push)
    leg = {'how': '64 slots, trained_d256, beam 10, %d frames per slot, the frames of a push start in a float32 device tensor '
                  '[64, n, 256]; one process per group and run, this commit and the parent interleaved, %d runs; '
                  'microseconds per push' % (a.frames, a.runs)}
    for per_push in (1, 16):
      tensors, today, host = (rows['%s_%d' % (k, per_push)] for k in ('push_tensors', 'today', 'host'))
      was = parent['host_%d' % per_push]
      leg['%d_frames_per_push' % per_push] = {
          'us_per_push': {'push_tensors': tensors, 'today': today, 'host': host, 'host_parent_commit': was},
          'median_us_per_push': {'push_tensors': _median(tensors), 'today': _median(today), 'host': _median(host),
                                 'host_parent_commit': _median(was)},
          'condition': _against(tensors, today, 'push_tensors against .double().cpu().numpy() + push'),
          'host_push_this_commit_against_the_parent': _against(host, was, 'push from a host array, this commit against the parent'),
          'labels_agree': len({r['labels_%s_%d' % (k, per_push)] for r in this_push for k in ('push_tensors', 'today', 'host')} |
                              {r['labels_host_%d' % per_push] for r in parent_push}) == 1}
    res['push'] = leg
  if decode:
    rows = _rows(decode)
    equal = rows.pop('labels_equal_predict')
    leg = {'how': '64 x 500 x 256, trained_d256, beam 10, test_iteration 2; the legs interleaved three times inside a process '
                  '(its median), %d processes; milliseconds per call, host clock around blocking calls' % a.runs,
           'ms_per_call': rows, 'median_ms_per_call': {k: _median(v) for k, v in rows.items()},
           'labels_equal_predict': all(equal)}
    for name in ('f64', 'f32', 'f16'):
      leg['condition_' + name] = _against(rows['predict_tensors_' + name], rows['today_' + name],
                                          'predict_tensors against .double().cpu().numpy() + predict, ' + name)
    leg['f64_against_predict_of_the_host_list'] = _against(rows['predict_tensors_f64'], rows['predict'],
                                                           'predict_tensors (float64) against predict of a list already on the host')
    leg['f32_against_decode_device'] = _against(rows['predict_tensors_f32'], rows['decode_device'],
                                                'predict_tensors (float32) against decode_device on the packed resident stream')
    res['decode'] = leg
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
