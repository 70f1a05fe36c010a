"""Primed decoding's CPU side: the restatement the GPU tests compare with, and the argument checks.

tests/primed_ref.py restates prime + look_ahead-1 beam search from the oracle's CoreRNN row and weighted MSE.
Checked here against the oracle's own decode (an empty prefix), against itself at beam 1 (priming with a greedy
decode's labels continues that decode), against a case with a known answer (a beam that never prunes holds exactly
the restricted-growth continuations of the prefix) and against the reference's run from a primed BeamState
(tests/golden/fn_primed.npz, recorded by tests/golden/make_primed.py).  No GPU needed.
"""

import os

import numpy as np
import pytest

import golden_util
import primed_ref
import uisrnn_amd
from uisrnn_amd import _capi
from uisrnn_amd import synth
from uisrnn_amd import uisrnn as host
from uisrnn_amd import weights


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2', 'tracker_d256'])
def test_an_empty_prefix_is_the_oracle_decode(name, oracle_lib):
  case = golden_util.load_case(name)
  seqs = case['seqs'][:2]
  for beam in (1, 3, 6, 10):
    ref = oracle_lib.decode(case['params'], seqs, beam, 1, 1, n_threads=2)
    for u, seq in enumerate(seqs):
      got = primed_ref.primed_decode(case['params'], seq, [], beam)
      assert np.array_equal(got['labels'][0], ref['labels'][u]), (beam, u)
      assert _bits(got['scores'][0]) == _bits(ref['scores'][u]), (beam, u)
      assert np.array_equal(_bits(primed_ref.padded_beam(got['scores'], beam)), _bits(ref['beam_scores'][u])), (beam, u)


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2'])
def test_beam_1_continues_its_own_decode(name, oracle_lib):
  case = golden_util.load_case(name)
  seq = case['seqs'][0]
  n = seq.shape[0]
  ref = oracle_lib.decode(case['params'], [seq], 1, 1, 1)
  for p in (1, 2, n - 1, n):
    got = primed_ref.primed_decode(case['params'], seq, ref['labels'][0][:p], 1)
    assert got['labels'].shape == (1, n)
    assert np.array_equal(got['labels'][0], ref['labels'][0]), p
    assert _bits(got['scores'][0]) == _bits(ref['scores'][0]), p


def _restricted_growth_continuations(prefix, n):
  """Every first-appearance continuation of `prefix` by n more frames."""
  out = [list(prefix)]
  for _ in range(n):
    out = [s + [c] for s in out for c in range(max(s) + 2)]
  return sorted(tuple(s) for s in out)


def test_a_beam_that_never_prunes_keeps_every_continuation(oracle_lib):
  case = golden_util.load_case('tiny_d16')
  seq = case['seqs'][0][:6]
  prefix = [0, 1, 1]   # K = 2, then n = 3 frames: 3 * 4 * 5 candidates at most, 3 + ... continuations
  want = _restricted_growth_continuations(prefix, 3)
  got = primed_ref.primed_decode(case['params'], seq, prefix, len(want))
  assert sorted(tuple(r) for r in got['labels'].tolist()) == want
  assert got['labels'].shape[0] == len(want) and np.all(np.diff(got['scores']) >= 0)
  # (the same count from tests/test_nbest_host.py's enumeration: the partitions of 6 frames that start with the prefix)
  import test_nbest_host  # pylint: disable=import-outside-toplevel
  assert want == [s for s in test_nbest_host.restricted_growth_strings(6) if list(s[:3]) == prefix]


@pytest.mark.parametrize('case', ['trained_toy4', 'trained_d256', 'd20_h24_depth3'])
def test_the_reference_from_a_primed_state(case, oracle_lib):
  data = np.load(os.path.join(golden_util.GOLDEN_DIR, 'fn_primed.npz'))
  assert sorted(str(c) for c in data['cases']) == ['d20_h24_depth3', 'trained_d256', 'trained_toy4']
  params = weights.load_checkpoint(os.path.join(golden_util.GOLDEN_DIR, str(data[case + '/checkpoint'])))
  lengths = [int(n) for n in data[case + '/lengths']]
  plen = [int(n) for n in data[case + '/prefix_lengths']]
  beam = int(data['beam_size'])
  assert beam == 5 and int(data[case + '/n_labelings']) == 2
  dim = int(params['observation_dim'])
  seqs = [synth.make_utterance(int(data[case + '/utt_seed']) + u, n, dim)[0] for u, n in enumerate(lengths)]
  bounds = np.concatenate([[0], np.cumsum(lengths)])
  for k in range(2):
    want = data['{}/labels_{}'.format(case, k)]
    for u, seq in enumerate(seqs):
      labels = want[bounds[u]:bounds[u + 1]]
      got = primed_ref.primed_decode(params, seq, labels[:plen[u]], beam)
      assert np.array_equal(got['labels'][0], labels), (case, k, u)
      np.testing.assert_allclose(got['scores'][0], data['{}/scores_{}'.format(case, k)][u], rtol=1e-4)
      np.testing.assert_allclose(got['prefix_score'], data['{}/prefix_scores_{}'.format(case, k)][u], rtol=1e-4)


class _StandIn:
  """A decoder that records what reaches it (no library, no device)."""

  def __init__(self, n_utt, have=None):
    self.have = np.zeros(n_utt, dtype=np.int64) if have is None else np.array(have, dtype=np.int64)
    self.calls = []

  def stream_received(self):
    return self.have.copy()

  def stream_prime(self, chunks, labels):
    self.calls.append((chunks, labels))
    return np.array([7.5 if lab is not None else 0.0 for lab in labels], dtype=np.float32)


def _session(n_utt, dim=4, have=None):
  model_args, _, _ = uisrnn_amd.parse_arguments([])
  model_args.observation_dim = dim
  session = host.OnlineSession.__new__(host.OnlineSession)  # (no handle: the checks come first)
  session._model = uisrnn_amd.UISRNN(model_args)
  session._num_utterances = n_utt
  session._decoder = _StandIn(n_utt, have)
  return session


def test_online_session_prime_argument_errors_need_no_device():
  session = _session(2, have=[0, 3])
  ok = np.zeros((3, 4))
  with pytest.raises(TypeError, match='numpy array of float type'):
    session.prime([ok.astype(np.float32), None], [[0, 0, 0], None])
  with pytest.raises(ValueError, match='2-dim'):
    session.prime([np.zeros(3), None], [[0, 0, 0], None])
  with pytest.raises(ValueError, match='observation_dim'):
    session.prime([np.zeros((3, 5)), None], [[0, 0, 0], None])
  with pytest.raises(ValueError):   # one entry per utterance
    session.prime([ok], [[0, 0, 0]])
  with pytest.raises(ValueError, match='2 ids for a prefix of 3 frames'):
    session.prime([ok, None], [[0, 0], None])
  with pytest.raises(ValueError, match='no frames'):
    session.prime([None, None], [[0], None])
  with pytest.raises(ValueError, match='already received 3 frames'):
    session.prime([None, ok], [None, [0, 0, 0]])
  with pytest.raises(TypeError):
    session.prime(ok, [0, 0, 0])
  assert not session._decoder.calls   # nothing reached the decoder
  # ids of any hashable kind are renamed by first appearance; None where nothing was primed
  got = session.prime([ok, None], [['bob', 'al', 'bob'], None])
  assert got == [7.5, None]
  chunks, labels = session._decoder.calls[0]
  assert chunks[1] is None and labels[1] is None and chunks[0] is ok
  assert labels[0].dtype == np.int32 and labels[0].tolist() == [0, 1, 0]
  # numpy ids, an empty prefix
  assert session.prime([ok, np.zeros((0, 4))], [np.array([5, 5, 2]), []]) == [7.5, None]
  assert session._decoder.calls[1][1][0].tolist() == [0, 0, 1]


def test_predict_primed_argument_errors_need_no_device():
  model_args, _, inference_args = uisrnn_amd.parse_arguments([])
  model_args.observation_dim = 16
  model = uisrnn_amd.UISRNN(model_args)  # (never fit or loaded: reaching the decoder would raise TypeError)
  seq = np.zeros((5, 16))
  inference_args.look_ahead, inference_args.test_iteration = 1, 1
  with pytest.raises(TypeError, match='either a list or numpy array'):
    model.predict_primed('nope', [], inference_args)
  with pytest.raises(TypeError, match='numpy array of float type'):
    model.predict_primed(seq.astype(np.float32), [0], inference_args)
  with pytest.raises(ValueError, match='2-dim'):
    model.predict_primed([np.zeros(5)], [[0]], inference_args)
  with pytest.raises(ValueError, match='one id sequence per test sequence'):
    model.predict_primed([seq], [[0], [0]], inference_args)
  with pytest.raises(ValueError, match='6 ids for a sequence of 5 frames'):
    model.predict_primed(seq, [0] * 6, inference_args)
  for look, tau in ((2, 1), (1, 2)):
    inference_args.look_ahead, inference_args.test_iteration = look, tau
    with pytest.raises(ValueError, match='look_ahead and test_iteration must be 1'):
      model.predict_primed(seq, [0], inference_args)
  inference_args.look_ahead, inference_args.test_iteration = 1, 1
  assert model.predict_primed([], [], inference_args) == []
  with pytest.raises(TypeError, match='transition_bias is None'):
    model.predict_primed(seq, [0], inference_args)


def test_the_symbol_is_declared_and_bound():
  assert 'uis_stream_prime' in _capi.EXPORTED_SYMBOLS
  header = open(os.path.join(os.path.dirname(golden_util.GOLDEN_DIR), '..', 'include', 'uisrnn_hip.h')).read()
  assert 'int32_t uis_stream_prime(uis_handle* h, const float* frames, const int64_t* offsets,' in header
  assert '#define UIS_ABI_VERSION 6' in header
