"""Record the reference's decode from a labeled prefix -> tests/golden/fn_primed.npz.

Runs only in the dev container: it imports the reference (make_golden.import_reference).  For every
utterance the prefix is replayed on the reference's own BeamState with its own _update_beam_state (as
make_trained.rescore_with_reference does), and the reference's predict_single then runs on the REMAINING
frames from that state: for the duration of the call the name BeamState in the reference's module yields
a copy of the primed state where predict_single asks for an empty one (its argument-less call) and is the
reference's class for every other use.  The reference's loop runs as it is; nothing of it is restated here.
The score recorded for a result is the reference's neg_likelihood of prefix + decoded labels, replayed the
same way.  Utterances are regenerated from synth seeds; only seeds, lengths, prefix lengths, labels and
scores are stored.  tests/test_prime_host.py and tests/test_gpu_prime.py read the file.

Labeling 0 of a case uses the synth truth as the prefix, labeling 1 random labels in 0 .. 2 (both renamed
by first appearance).  beam_size 5, look_ahead 1, test_iteration 1.

The utterance seeds below are the first tried; had a near-tie made tests/primed_ref.py differ from the
reference on the CPU (the script checks when the oracle library is available and says so), the rule is
to move to the next seed before recording, and to note it here.

  python tests/golden/make_primed.py
"""

import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, _HERE)
sys.path.insert(0, os.path.dirname(_HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))

import make_golden  # noqa: E402  pylint: disable=wrong-import-position
import make_trained  # noqa: E402  pylint: disable=wrong-import-position
from uisrnn_amd import synth, weights  # noqa: E402  pylint: disable=wrong-import-position

OUT = os.path.join(_HERE, 'fn_primed.npz')  # (fn_: kept out of golden_util.case_names, like make_forced.py's)
BEAM = 5

# case -> (checkpoint, utterance seed, lengths, prefix lengths)
CASES = {
    'trained_toy4': ('trained_toy4.uisrnn', 9600, [50, 30], [12, 9]),
    'trained_d256': ('trained_d256.uisrnn', 9700, [60, 40], [20, 15]),
    'd20_h24_depth3': ('d20_h24_depth3.uisrnn', 9800, [50, 35], [10, 1]),
}


def first_appearance(ids):
  names = {}
  return [names.setdefault(int(i), len(names)) for i in ids]


def primed_state(ref, model, seq, prefix):
  """The reference's BeamState after `prefix` along the first frames of seq."""
  import torch  # pylint: disable=import-outside-toplevel
  frames = torch.autograd.Variable(torch.from_numpy(seq).float())
  state = ref.BeamState()
  with torch.no_grad():
    for t, cluster in enumerate(prefix):
      state = model._update_beam_state(state, frames[t:t + 1, :], [int(cluster)])  # pylint: disable=protected-access
  return state


def decode_from(ref, model, state, rest, inference_args):
  """predict_single over `rest` with `state` where it would start from an empty BeamState."""
  import torch  # pylint: disable=import-outside-toplevel
  real = ref.BeamState

  def beam_state(source=None):
    return real(state) if source is None else real(source)

  ref.BeamState = beam_state
  try:
    with torch.no_grad():
      return [int(c) for c in model.predict_single(rest, inference_args)]
  finally:
    ref.BeamState = real


def main():
  uisrnn = make_golden.import_reference()
  import uisrnn.uisrnn as ref  # pylint: disable=import-outside-toplevel
  rng = np.random.default_rng(0)
  record = {'cases': np.array(sorted(CASES)), 'beam_size': np.int64(BEAM)}
  for case in sorted(CASES):
    ckpt, seed, lengths, prefix_lens = CASES[case]
    path = os.path.join(_HERE, ckpt)
    params = weights.load_checkpoint(path)
    model_args, _, inference_args = make_trained._args(uisrnn)  # pylint: disable=protected-access
    model_args.enable_cuda = False
    model_args.verbosity = 0
    model_args.observation_dim = int(params['observation_dim'])
    model_args.rnn_hidden_size = int(params['rnn_hidden_size'])
    model_args.rnn_depth = int(params['rnn_depth'])
    inference_args.beam_size, inference_args.look_ahead, inference_args.test_iteration = BEAM, 1, 1
    model = make_trained._load_reference_model(uisrnn, model_args, path)  # pylint: disable=protected-access
    model.rnn_model.eval()  # as predict_single does (uisrnn.py:523): no dropout between GRU layers
    dim = int(params['observation_dim'])
    seqs, truths = zip(*[synth.make_utterance(seed + u, n, dim) for u, n in enumerate(lengths)])
    prefixes = [[first_appearance(list(t)[:p]) for t, p in zip(truths, prefix_lens)],
                [first_appearance(rng.integers(0, 3, size=p)) for p in prefix_lens]]
    record[case + '/checkpoint'] = np.array(ckpt)
    record[case + '/utt_seed'] = np.int64(seed)
    record[case + '/lengths'] = np.array(lengths, dtype=np.int64)
    record[case + '/prefix_lengths'] = np.array(prefix_lens, dtype=np.int64)
    record[case + '/n_labelings'] = np.int64(len(prefixes))
    for k, per_utt in enumerate(prefixes):
      labels, scores, prefix_scores = [], [], []
      for seq, prefix in zip(seqs, per_utt):
        state = primed_state(ref, model, seq, prefix)
        decoded = decode_from(ref, model, state, seq[len(prefix):], inference_args)
        assert len(decoded) == seq.shape[0] - len(prefix)
        full = list(prefix) + decoded
        labels.append(full)
        prefix_scores.append(float(state.neg_likelihood))
        scores.append(make_trained.rescore_with_reference(model, seq, full, 1))
      record['{}/labels_{}'.format(case, k)] = np.concatenate(labels).astype(np.int32)
      record['{}/scores_{}'.format(case, k)] = np.array(scores, dtype=np.float64)
      record['{}/prefix_scores_{}'.format(case, k)] = np.array(prefix_scores, dtype=np.float64)
      print(case, k, scores, prefix_scores)
      try:  # (a look at the CPU restatement before anything is written: see the note on seeds above)
        import primed_ref  # pylint: disable=import-outside-toplevel
        for seq, prefix, full in zip(seqs, per_utt, labels):
          got = primed_ref.primed_decode(params, seq, prefix, BEAM)['labels'][0].tolist()
          print('  primed_ref', 'agrees' if got == full else 'DIFFERS: choose another seed')
      except (ImportError, OSError) as err:
        print('  primed_ref not checked:', err)
  np.savez_compressed(OUT, **record)
  print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
  main()
