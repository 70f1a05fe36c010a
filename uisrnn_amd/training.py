"""Host side of training: data preparation and the iteration loop around the HIP trainer.

The behaviour is the reference's ``UISRNN.fit`` / ``fit_concatenated`` (uisrnn/uisrnn.py:172-386)
and the helpers of uisrnn/utils.py they call.  Everything that draws random numbers here makes
the same calls on Python's ``random`` and the global ``np.random``, in the same order, as the
reference: a caller who seeds both gets the reference's batch sequence exactly.

The arithmetic of each iteration (GRU forward, losses, backward, clipping, Adam) runs in
libuisrnn_hip.so (uisrnn_amd/csrc/uis_train.hip) through ``_capi.Trainer``.

Deviations from the reference:
  * ``batch_size=None`` trains on one full batch of all sub-sequences; the reference accepts the
    value but fails at ``rnn_init_hidden.repeat(1, None, 1)``.
  * Dropout between GRU layers (``rnn_depth >= 2`` and ``rnn_dropout > 0``) uses the trainer's own
    counter-based random stream, keyed once per call by ``random.getrandbits(64)`` drawn after the
    permutations.  Its masks cannot match torch's.  The ``np.random`` stream stays aligned with the
    reference's; Python's ``random`` does too wherever no dropout applies (that draw is its only
    extra use).
"""

import random
import string

import numpy as np

_ID_ALPHABET = string.ascii_uppercase + string.digits


def estimate_transition_bias(cluster_ids, smooth=1):
  """(bias, bias_denominator): the smoothed share of speaker changes between neighbours.

  cluster_ids is a list of label sequences (or one concatenated sequence inside a list).
  """
  changes = smooth
  pairs = 2 * smooth
  for seq in cluster_ids:
    for a, b in zip(seq[:-1], seq[1:]):
      changes += (a != b)
      pairs += 1
  return changes / pairs, pairs


def merge_transition_bias(old_bias, old_denominator, bias, denominator):
  """A further fit()'s estimate weighted into the model's (uisrnn/uisrnn.py:367-375)."""
  if old_bias is None:
    return bias, denominator
  merged = (old_bias * old_denominator + bias * denominator) / (old_denominator + denominator)
  return merged, old_denominator + denominator


def _random_id(length=6):
  return ''.join([random.choice(_ID_ALPHABET) for _ in range(length)])


def enforce_cluster_id_uniqueness(cluster_ids):
  """Prefix every sequence's labels with a random 6-character id of its own."""
  if not isinstance(cluster_ids, list):
    raise TypeError('cluster_ids must be a list')
  out = []
  for labels in cluster_ids:
    prefix = _random_id()
    if isinstance(labels, np.ndarray):
      labels = labels.tolist()
    if not isinstance(labels, list):
      raise TypeError('Elements of cluster_ids must be list or numpy.ndarray')
    out.append([prefix + '_' + s for s in labels])
  return out


def _first_failure(checks):
  """Raise the exception of the first (failed, exception) pair whose condition holds."""
  for failed, error in checks:
    if failed():
      raise error


def _as_label_list(labels):
  return labels.tolist() if isinstance(labels, np.ndarray) else labels


def _check_training_lists(train_sequences, train_cluster_ids):
  """Argument errors of the reference's concatenate_training_data, in its order."""
  _first_failure([
      (lambda: not (isinstance(train_sequences, list) and isinstance(train_cluster_ids, list)),
       TypeError('train_sequences and train_cluster_ids must be lists')),
      (lambda: len(train_sequences) != len(train_cluster_ids),
       ValueError('train_sequences and train_cluster_ids must have same size')),
  ])
  dims = set()
  for seq, labels in zip(train_sequences, train_cluster_ids):
    rows, dim = seq.shape
    dims.add(dim)
    _first_failure([
        (lambda: len(dims) > 1,
         ValueError('train_sequences must have consistent observation dimension')),
        (lambda: not isinstance(labels, list),
         TypeError('Elements of train_cluster_ids must be list or numpy.ndarray')),
        (lambda: len(labels) != rows,
         ValueError('Each train_sequence and its train_cluster_id must have same length')),
    ])


def concatenate_training_data(train_sequences, train_cluster_ids,
                              enforce_uniqueness=True, shuffle=True):
  """Validate, make labels unique per sequence, shuffle the sequences, concatenate.

  Returns (the [N, D] concatenation, its N labels as a list).
  """
  if isinstance(train_cluster_ids, list):
    train_cluster_ids = list(map(_as_label_list, train_cluster_ids))
  _check_training_lists(train_sequences, train_cluster_ids)
  if enforce_uniqueness:
    train_cluster_ids = enforce_cluster_id_uniqueness(train_cluster_ids)
  order = list(zip(train_sequences, train_cluster_ids))
  if shuffle:
    random.shuffle(order)
  sequence = np.concatenate([seq for seq, _ in order], axis=0)
  labels = []
  for _, ids in order:
    labels.extend(ids)
  return sequence, labels


def sample_permuted_segments(index_sequence, number_samples):
  """number_samples orderings of index_sequence's runs of consecutive indices, each a fresh
  np.random.permutation of the runs."""
  n = len(index_sequence)
  if n == 1:
    runs = [index_sequence]
  else:
    cuts = [i + 1 for i in range(n - 1) if index_sequence[i + 1] != index_sequence[i] + 1]
    bounds = [0] + cuts + [n]
    runs = [index_sequence[a:b] for a, b in zip(bounds[:-1], bounds[1:])]
  samples = []
  for _ in range(number_samples):
    order = np.random.permutation(len(runs))
    samples.append(np.concatenate([runs[k] for k in order]))
  return samples


def resize_sequence(sequence, cluster_id, num_permutations=None):
  """One sub-sequence per cluster (or num_permutations run-permuted copies of it).

  Returns (sub_sequences, seq_lengths) with seq_lengths = rows + 1, clusters in np.unique order.
  """
  cluster_id = np.asarray(cluster_id)
  sub_sequences, seq_lengths = [], []
  for label in np.unique(cluster_id):
    rows = np.where(cluster_id == label)[0]
    if num_permutations and num_permutations > 1:
      for order in sample_permuted_segments(rows, num_permutations):
        sub_sequences.append(sequence[order, :])
        seq_lengths.append(len(rows) + 1)
    else:
      sub_sequences.append(sequence[rows, :])
      seq_lengths.append(len(rows) + 1)
  return sub_sequences, seq_lengths


def length_order(seq_lengths):
  """(sorted lengths, sub-sequence index) in non-increasing length order, tie order included."""
  return np.sort(seq_lengths)[::-1], np.argsort(seq_lengths)[::-1]


def draw_batch(num_clusters, batch_size):
  """Positions (into length_order) of one mini-batch: drawn with replacement, sorted."""
  return np.sort(np.random.choice(num_clusters, batch_size))


class BatchPlan:
  """The sub-sequences in length order and each iteration's batch, as the reference packs them."""

  def __init__(self, seq_lengths, batch_size):
    self.sorted_lengths, self.order = length_order(seq_lengths)
    self.batch_size = batch_size

  def next(self):
    """Sub-sequence indices of the next iteration's batch, longest first."""
    if self.batch_size is None:
      return self.order.astype(np.int32)
    picks = draw_batch(len(self.order), self.batch_size)
    return self.order[picks].astype(np.int32)


def prepare(train_sequence, train_cluster_id, num_permutations, batch_size):
  """fit_concatenated's data preparation: (sub_sequences, BatchPlan).  Draws the permutations."""
  sub_sequences, seq_lengths = resize_sequence(train_sequence, train_cluster_id, num_permutations)
  return sub_sequences, BatchPlan(seq_lengths, batch_size)


def padded_batch(sub_sequences, batch_idx):
  """The padded [T, B, D] input of one batch, on the host (what the device gathers)."""
  lengths = [len(sub_sequences[i]) + 1 for i in batch_idx]
  dim = sub_sequences[batch_idx[0]].shape[1]
  out = np.zeros((lengths[0], len(batch_idx), dim), dtype=np.float32)
  for b, i in enumerate(batch_idx):
    out[1:lengths[b], b, :] = sub_sequences[i]
  return out


def check_concatenated(train_sequence, train_cluster_id, observation_dim):
  """Argument errors of the reference's fit_concatenated, in its order; returns the labels as an array."""
  if isinstance(train_cluster_id, list):
    train_cluster_id = np.array(train_cluster_id)
  is_float_array = isinstance(train_sequence, np.ndarray) and train_sequence.dtype == float
  is_string_array = (isinstance(train_cluster_id, np.ndarray) and
                     train_cluster_id.dtype.kind == 'U')
  _first_failure([
      (lambda: not is_float_array,
       TypeError('train_sequence should be a numpy array of float type.')),
      (lambda: not is_string_array,
       TypeError('train_cluster_id type be a numpy array of strings.')),
      (lambda: train_sequence.ndim != 2,
       ValueError('train_sequence must be 2-dim array.')),
      (lambda: train_cluster_id.ndim != 1,
       ValueError('train_cluster_id must be 1-dim array.')),
      (lambda: train_sequence.shape[1] != observation_dim,
       ValueError('train_sequence does not match the dimension specified by '
                  'args.observation_dim.')),
      (lambda: train_sequence.shape[0] != len(train_cluster_id),
       ValueError('train_sequence length is not equal to train_cluster_id length.')),
  ])
  return train_cluster_id


def train_concatenated(model, train_sequence, train_cluster_id, args, log):
  """fit_concatenated on the device: returns (new params, per-iteration loss records)."""
  from uisrnn_amd import _capi  # pylint: disable=import-outside-toplevel
  train_cluster_id = check_concatenated(train_sequence, train_cluster_id, model.observation_dim)
  if getattr(args, 'optimizer', 'adam') != 'adam':
    raise AssertionError('Only adam optimizer is supported.')
  sub_sequences, plan = prepare(train_sequence, train_cluster_id, args.num_permutations,
                                args.batch_size)
  # Python's random is drawn only where dropout applies: elsewhere the stream stays the reference's
  dropout = model.rnn_dropout if model.params['rnn_depth'] >= 2 else 0.0
  dropout_key = random.getrandbits(64) if dropout > 0 else 0
  trainer = _capi.Trainer(
      model.params, device=model.device_index,
      learning_rate=args.learning_rate,
      regularization_weight=args.regularization_weight,
      grad_max_norm=args.grad_max_norm,
      sigma_alpha=args.sigma_alpha, sigma_beta=args.sigma_beta,
      estimate_sigma2=model.estimate_sigma2,
      dropout=dropout, dropout_key=dropout_key)
  records = []
  try:
    trainer.set_data(sub_sequences)
    for num_iter in range(args.train_iteration):
      loss, loss1, loss2, loss3 = trainer.step(plan.next())
      records.append({'loss': loss, 'loss1': loss1, 'loss2': loss2, 'loss3': loss3})
      if num_iter % 10 == 0 or num_iter == args.train_iteration - 1:
        log(2, 'Iter: {:d}  \t'
               'Training Loss: {:.4f}    \n'
               '    Negative Log Likelihood: {:.4f}\t'
               'Sigma2 Prior: {:.4f}\t'
               'Regularization: {:.4f}'.format(num_iter, loss, loss1, loss2, loss3))
    log(1, 'Done training with {} iterations'.format(args.train_iteration))
    params = trainer.params()
  finally:
    trainer.close()
  return params, records
