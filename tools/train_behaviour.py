"""The reference's two behavioural training tests, run through train(), and a sweep over seeds.

  python tools/train_behaviour.py [--seeds 20]

single_label: tests/uisrnn_test.py of the reference -- 1000 frames of one label, 50 iterations;
  predict must give [0] * 10 for an array, a list and parallel_predict.
four_clusters: tests/integration_test.py of the reference -- four clusters on a square, depth 2
  with the default dropout 0.2, 200 iterations; accuracy must be 1.0, also after save / load.

The starting weights come from weights.init_params(seed=weight_seed); the data and batches from
np.random / random seeded with 1, as in the reference's tests.  The sweep prints, for each
weight seed, whether each case passes (tests/test_gpu_train.py runs weight seed 0).
"""

import argparse
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import uisrnn_amd  # noqa: E402  pylint: disable=wrong-import-position
from uisrnn_amd import weights  # noqa: E402  pylint: disable=wrong-import-position


def _seeded_model(model_args, weight_seed):
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(weights.init_params(
      model_args.observation_dim, model_args.rnn_hidden_size, model_args.rnn_depth,
      sigma2=model_args.sigma2, transition_bias=model_args.transition_bias,
      crp_alpha=model_args.crp_alpha, seed=weight_seed))
  return model


def single_label(weight_seed):
  """(model, predict on an array, on a list, through parallel_predict)."""
  np.random.seed(1)
  random.seed(1)
  model_args, training_args, inference_args = uisrnn_amd.parse_arguments([])
  model_args.rnn_depth, model_args.rnn_hidden_size, model_args.observation_dim = 1, 8, 16
  model_args.verbosity = 0
  training_args.learning_rate = 0.01
  training_args.train_iteration = 50
  model = _seeded_model(model_args, weight_seed)
  model.train(np.random.rand(1000, 16), np.array(['A'] * 1000), training_args)
  one = model.predict(np.random.rand(10, 16) / 10.0, inference_args)
  seqs = [np.random.rand(10, 16) / 10.0 for _ in range(3)]
  many = model.predict(seqs, inference_args)
  par = uisrnn_amd.parallel_predict(model, seqs, inference_args, num_processes=2)
  return model, one, many, par


def _square(ids, sigma):
  centers = {'A': (0.0, 0.0), 'B': (0.0, 1.0), 'C': (1.0, 0.0), 'D': (1.0, 1.0)}
  pts = np.array([centers[i] for i in ids])
  return pts + np.random.rand(*pts.shape) * sigma


def four_clusters(weight_seed):
  """(model, training data, test sequence, test labels, inference args, predicted labels)."""
  np.random.seed(1)
  random.seed(1)
  train_id = ['A'] * 400 + ['B'] * 300 + ['C'] * 200 + ['D'] * 100
  random.shuffle(train_id)
  train_seq = _square(train_id, 0.01)
  cuts = [0, 100, 300, 600, 1000]
  train_seqs = [train_seq[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
  train_ids = [train_id[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
  test_id = ['A'] * 10 + ['B'] * 20 + ['C'] * 30 + ['D'] * 40
  random.shuffle(test_id)
  test_seq = _square(test_id, 0.01)
  model_args, training_args, inference_args = uisrnn_amd.parse_arguments([])
  model_args.rnn_depth, model_args.rnn_hidden_size, model_args.observation_dim = 2, 8, 2
  model_args.verbosity = 0
  training_args.learning_rate = 0.01
  training_args.train_iteration = 200
  training_args.enforce_cluster_id_uniqueness = False
  inference_args.test_iteration = 2
  model = _seeded_model(model_args, weight_seed)
  model.train(train_seqs, train_ids, training_args)
  labels = model.predict(test_seq, inference_args)
  return model, (train_seqs, train_ids, training_args), test_seq, test_id, inference_args, labels


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--seeds', type=int, default=20)
  a = ap.parse_args()
  rows = []
  for seed in range(a.seeds):
    _, one, many, par = single_label(seed)
    single_ok = one == [0] * 10 and many == [[0] * 10] * 3 and par == many
    _, _, _, test_id, _, labels = four_clusters(seed)
    acc = uisrnn_amd.compute_sequence_match_accuracy(labels, test_id)
    rows.append({'weight_seed': seed, 'single_label_ok': bool(single_ok), 'four_clusters_accuracy': acc})
    print(json.dumps(rows[-1]), flush=True)
  print(json.dumps({'seeds': a.seeds,
                    'single_label_pass': sum(r['single_label_ok'] for r in rows),
                    'four_clusters_accuracy_1': sum(r['four_clusters_accuracy'] == 1.0 for r in rows)}))


if __name__ == '__main__':
  main()
