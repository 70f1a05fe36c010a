"""Record the reference's neg_likelihood of given labelings -> tests/golden/fn_forced_scores.npz.

Runs only in the dev container: it imports the reference (make_golden.import_reference) and replays
uisrnn/uisrnn.py:388-453 along each labeling with make_trained.rescore_with_reference, test_iteration 1.
Utterances are regenerated from synth seeds; only labels and scores are stored.  tests/test_gpu_score.py
reads the file.

  python tests/golden/make_forced.py
"""

import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, _HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))

import make_golden  # noqa: E402  pylint: disable=wrong-import-position
import make_trained  # noqa: E402  pylint: disable=wrong-import-position
from uisrnn_amd import synth, weights  # noqa: E402  pylint: disable=wrong-import-position

OUT = os.path.join(_HERE, 'fn_forced_scores.npz')  # (fn_: kept out of golden_util.case_names, like make_scores.py's)

# case -> (checkpoint, utterance seed, lengths)
CASES = {
    'trained_single': ('trained_single.uisrnn', 9100, [40, 25]),
    'trained_toy4': ('trained_toy4.uisrnn', 9200, [50, 30]),
    'trained_d256': ('trained_d256.uisrnn', 9300, [80, 60]),
    'trained_d512': ('trained_d512.uisrnn', 9400, [60, 40]),
    'd20_h24_depth3': ('d20_h24_depth3.uisrnn', 9500, [50, 35]),
}


def first_appearance(ids):
  names = {}
  return [names.setdefault(int(i), len(names)) for i in ids]


def labelings(truth, rng):
  """Truth, truth with a few frames moved to another (or a new) cluster, and a random labeling."""
  out = [first_appearance(truth)]
  moved = list(truth)
  for t in rng.choice(len(moved), size=max(1, len(moved) // 10), replace=False):
    moved[t] = int(rng.integers(0, max(moved) + 2))
  out.append(first_appearance(moved))
  out.append(first_appearance(rng.integers(0, 3, size=len(truth))))
  return out


def main():
  uisrnn = make_golden.import_reference()
  rng = np.random.default_rng(0)
  record = {'cases': np.array(sorted(CASES))}
  for case in sorted(CASES):
    ckpt, seed, lengths = CASES[case]
    path = os.path.join(_HERE, ckpt)
    params = weights.load_checkpoint(path)
    model_args, _, _ = make_trained._args(uisrnn)  # pylint: disable=protected-access
    model_args.enable_cuda = False
    model_args.verbosity = 0
    model_args.observation_dim = int(params['observation_dim'])
    model_args.rnn_hidden_size = int(params['rnn_hidden_size'])
    model_args.rnn_depth = int(params['rnn_depth'])
    model = make_trained._load_reference_model(uisrnn, model_args, path)  # pylint: disable=protected-access
    model.rnn_model.eval()  # as predict_single does (uisrnn.py:523): no dropout between GRU layers
    dim = int(params['observation_dim'])
    seqs, truths = zip(*[synth.make_utterance(seed + u, n, dim) for u, n in enumerate(lengths)])
    per_utt = [labelings(list(t), rng) for t in truths]
    n_lab = len(per_utt[0])
    record[case + '/checkpoint'] = np.array(ckpt)
    record[case + '/utt_seed'] = np.int64(seed)
    record[case + '/lengths'] = np.array(lengths, dtype=np.int64)
    record[case + '/n_labelings'] = np.int64(n_lab)
    for k in range(n_lab):
      labels = [per_utt[u][k] for u in range(len(seqs))]
      scores = [make_trained.rescore_with_reference(model, s, lab, 1) for s, lab in zip(seqs, labels)]
      record['{}/labels_{}'.format(case, k)] = np.concatenate(labels).astype(np.int32)
      record['{}/scores_{}'.format(case, k)] = np.array(scores, dtype=np.float64)
      print(case, k, scores)
  np.savez_compressed(OUT, **record)
  print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
  main()
