"""Primed sessions (uis_stream_prime): online decoding that starts from a labeled prefix.

The contract of include/uisrnn_hip.h: after priming, a session is in the state it would hold had it received the
prefix frames with its beam holding only the given labeling.  Checked bit for bit -- labels, scores, the whole final
beam as uint32 -- against
  - the offline decode and the CPU oracle where the prefix is the beam-1 decode's own labels (a greedy decode
    continues exactly where it was), on every session path;
  - tests/primed_ref.py, the CPU restatement of prime + beam search, for wider beams and arbitrary prefixes;
  - the reference's own run from a primed BeamState (tests/golden/fn_primed.npz): labels identical, scores 1e-4;
and: a persistent session, every refusal (the session must be left as it was), UIS_POISON_WORKSPACE, and the Python
layer (UISRNN.predict_primed).
"""

import functools
import os

import numpy as np
import pytest

import golden_util
import primed_ref
import test_gpu_hostile as gh
import uisrnn_amd
from oracle import oracle
from uisrnn_amd import _capi
from uisrnn_amd import synth
from uisrnn_amd import weights

pytestmark = pytest.mark.gpu

WORDS = ('ffffffff', '7f7f7f7f', '80000000')
KNOB = 'UIS_POISON_WORKSPACE'
LENS = [60, 33, 1, 90, 17, 45, 72, 8, 64]


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _env(monkeypatch, word):
  """tests/test_gpu_poison.py::_env: the knob (None: unset), the arena layout."""
  if word is None:
    monkeypatch.delenv(KNOB, raising=False)
  else:
    monkeypatch.setenv(KNOB, word)
  monkeypatch.delenv('UIS_NO_ARENA', raising=False)


def _first_appearance(ids):
  names = {}
  return np.array([names.setdefault(int(i), len(names)) for i in ids], dtype=np.int32)


def _info(dec, n_utt, beam):
  info = np.empty((n_utt, beam), dtype=np.float32)
  dec._check(dec._lib.uis_last_decode_info(dec._handle, None, info.ctypes.data_as(_capi._fp)), 'info')  # pylint: disable=protected-access
  return info


def _random_schedule(rng, lens, max_chunk):
  left = list(lens)
  schedule = []
  while any(left):
    counts = []
    for u, n in enumerate(left):
      take = int(min(n, rng.integers(0, max_chunk + 1)))   # 0 = this utterance is silent in this push
      counts.append(take)
      left[u] -= take
    if any(counts):
      schedule.append(counts)
  return schedule


def _primed_stream(dec, seqs, prefixes, beam, schedule, max_frames, flags=0, max_clusters=0, after=None):
  """Open a session, prime every utterance with its prefix, push the rest by `schedule` (frame counts per push and
  utterance).  after(dec, pos): called right after priming and after every push.  Returns (labels, scores,
  overflow, status, final beam, prefix scores)."""
  dec.stream_begin(len(seqs), beam, max_frames, max_clusters=max_clusters, flags=flags)
  try:
    pos = [len(p) for p in prefixes]
    primed = dec.stream_prime([seqs[u][:pos[u]] if pos[u] else None for u in range(len(seqs))],
                              [p if len(p) else None for p in prefixes])
    if after is not None:
      after(dec, pos)
    for counts in schedule:
      chunks = []
      for u, n in enumerate(counts):
        chunks.append(seqs[u][pos[u]:pos[u] + n] if n else None)
        pos[u] += n
      dec.stream_push(chunks)
      if after is not None:
        after(dec, pos)
    assert pos == [len(s) for s in seqs], 'schedule does not cover the utterances'
    labels, scores, overflow, status = dec.stream_labels()
    return labels, scores, overflow, status, _info(dec, len(seqs), beam), primed
  finally:
    dec.stream_end()


# ---- 1. greedy continuation, every session path

def _model(name):
  if name == 'tracker_256_512':
    return synth.tracker_params(256, 512, 1, seed=21)
  if name == 'tracker_256_256':
    return synth.tracker_params(256, 256, 1, seed=25)
  if name == 'tracker_d64_h300':
    return golden_util.load_case('tracker_d64_h300')['params']
  if name == 'init_33_17_2':
    # (sigma2 0.01: at the constructor's 0.1 a fresh model's greedy decode never opens a second cluster; seed 177: of
    # the seeds 173 .. 178 one whose greedy decode also comes BACK to a cluster inside a prefix -- it opens up to 16)
    return weights.init_params(33, 17, 2, sigma2=0.01, transition_bias=0.2, crp_alpha=1.0, seed=177)
  return golden_util.load_case('d20_h24_depth3')['params']


@functools.lru_cache(maxsize=None)
def _greedy(name):
  """(params, 18 utterances, the oracle's beam-1 decode, prefix lengths), shared by the tests on this data."""
  oracle.lib()
  params = _model(name)
  dim = int(params['observation_dim'])
  seqs = (synth.make_utterances(12_000, len(LENS), LENS, dim)[0] +
          synth.make_utterances(12_500, len(LENS), LENS, dim)[0])
  # (d20_h24_depth3 -- sigma2 0.08 in 20 dimensions -- keeps unit-norm speakers in ONE cluster whatever the seed: its
  # utterances are the same synth ones at six times the amplitude, where its greedy decode does switch)
  seqs = [s * AMPLITUDE.get(name, 1.0) for s in seqs]
  ref = oracle.decode(params, seqs, 1, 1, 1, n_threads=8)
  cycle = [lambda n: 0, lambda n: 1, lambda n: 2, lambda n: n, lambda n: n - 1, lambda n: n // 2]
  plen = [min(max(cycle[u % 6](len(s)), 0), len(s)) for u, s in enumerate(seqs)]
  return params, seqs, ref, plen


def _chain_facts(prefixes):
  """(chains, most clusters in a prefix, largest block count) of a list of prefixes."""
  chains, most, blocks = 0, 0, 0
  for p in prefixes:
    k = int(p.max()) + 1 if len(p) else 0
    chains += k
    most = max(most, k)
    for c in range(k):
      on = np.concatenate([[0], (np.asarray(p) == c).astype(np.int64)])
      blocks = max(blocks, int((np.diff(on) == 1).sum()))
  return chains, most, blocks


AMPLITUDE = {'d20_h24_depth3': 6.0}
CLUSTER_CAP = {'init_33_17_2': 24}   # (max_clusters of the decode and the sessions; 0: the default 16)
# UIS_FLAG_RESIDENT in a session of this model (18 utterances, beam 1): True = the one-launch kernel must take it
# (rnn_depth 1 at hidden size 256 / 512 -- hidden 300 is embedded in the 512-wide kernels), False = uis_stream_begin
# must refuse it with UIS_ERR_UNSUPPORTED (rnn_depth >= 2: sessions have no one-launch kernel for it)
RESIDENT_SESSION = {'tracker_256_512': True, 'tracker_256_256': True, 'tracker_d64_h300': True,
                    'init_33_17_2': False, 'd20_h24_depth3': False}
GREEDY_MODELS = ['tracker_256_512', 'tracker_256_256', 'tracker_d64_h300', 'init_33_17_2', 'd20_h24_depth3']


def _greedy_case(name, dec, flag_sets, rng_seed=0):
  params, seqs, ref, plen = _greedy(name)
  del params
  prefixes = [ref['labels'][u][:plen[u]] for u in range(len(seqs))]
  # the test's own inputs: a second 16-row tile of the chain kernels, a prefix of three clusters, a cluster that
  # was left and come back to
  chains, most, blocks = _chain_facts(prefixes)
  assert chains > 16, chains
  assert most >= 3, most
  assert blocks >= 2, blocks
  frames, offsets = oracle.pack(seqs)
  cap = CLUSTER_CAP.get(name, 0)
  off = dec.decode(frames, offsets, 1, 1, 1, max_clusters=cap, want_beam_scores=True)
  assert off['status'] == 0 and not off['overflow'].any()
  rest = [len(s) - p for s, p in zip(seqs, plen)]
  schedule = _random_schedule(np.random.default_rng(rng_seed), rest, 7)
  for flags in flag_sets:
    if flags == _capi.UIS_FLAG_RESIDENT and not RESIDENT_SESSION[name]:
      with pytest.raises(_capi.HipLibraryError) as err:
        dec.stream_begin(len(seqs), 1, max(LENS), max_clusters=cap, flags=flags)
      assert err.value.status == _capi.UIS_ERR_UNSUPPORTED, name
      continue
    labels, scores, overflow, status, beam, primed = _primed_stream(dec, seqs, prefixes, 1, schedule, max(LENS), flags=flags,
                                                                      max_clusters=cap)
    assert status == 0 and not overflow.any(), flags
    for u in range(len(seqs)):
      assert np.array_equal(labels[u], off['labels'][offsets[u]:offsets[u + 1]]), (flags, u, plen[u])
      assert np.array_equal(labels[u], ref['labels'][u]), (flags, u, plen[u])
      if plen[u] == len(seqs[u]):   # primed with everything: the prefix's NLL is the decode's score
        assert _bits(primed[u]) == _bits(off['scores'][u]), (flags, u)
    assert np.array_equal(_bits(scores), _bits(off['scores'])), flags
    assert np.array_equal(_bits(beam), _bits(off['beam_scores'])), flags
    assert np.array_equal(_bits(beam), _bits(ref['beam_scores'])), flags


@pytest.mark.parametrize('name', GREEDY_MODELS)
def test_greedy_continuation_on_every_session_path(name, oracle_lib):
  dec = _capi.Decoder(_greedy(name)[0])
  _greedy_case(name, dec, (_capi.UIS_FLAG_RESIDENT, _capi.UIS_FLAG_STEPWISE, 0))
  dec.close()


# ---- 2. beam search from a primed state

@functools.lru_cache(maxsize=None)
def _beam_data(name):
  """(params, utterances, prefixes): synth truth, random labels for a third, a 1-frame prefix, chains of 1 and 2
  frames, and (256 / 512) one utterance that is not primed at all."""
  rng = np.random.default_rng(31)
  if name == 'tracker_256_512':
    params, dim = synth.tracker_params(256, 512, 1, seed=21), 256
    lens = [12, 9, 10, 5, 7, 8, 3, 9]
  else:
    params, dim = _model('init_33_17_2'), 33
    lens = [12, 9, 10, 5, 7, 8]
  # (speaker turns of three frames on average: at synth's default of twenty a five-frame truth prefix has one speaker)
  seqs, truth = zip(*[synth.make_utterance(12_800 + u, n, dim, mean_segment=3.0) for u, n in enumerate(lens)])
  seqs = list(seqs)
  prefixes = [_first_appearance(truth[0][:5]),
              _first_appearance(rng.integers(0, 3, size=4)),
              _first_appearance(rng.integers(0, 3, size=4)),
              np.array([0], dtype=np.int32),
              np.array([0, 1, 1], dtype=np.int32),
              _first_appearance(truth[5][:4])]
  if len(lens) > 6:
    prefixes += [_first_appearance(truth[6][:2]), np.zeros(0, dtype=np.int32)]
  assert len(prefixes) == len(lens)
  return params, seqs, prefixes


@functools.lru_cache(maxsize=None)
def _beam_ref(name, beam):
  oracle.lib()
  params, seqs, prefixes = _beam_data(name)
  return [primed_ref.primed_decode(params, s, p, beam) for s, p in zip(seqs, prefixes)]


def _check_against_ref(ref, beam, labels, scores, info, what=''):
  for u, r in enumerate(ref):
    assert np.array_equal(labels[u], r['labels'][0]), (what, u)
    assert _bits(scores[u]) == _bits(r['scores'][0]), (what, u)
    assert np.array_equal(_bits(info[u]), _bits(primed_ref.padded_beam(r['scores'], beam))), (what, u)


def _beam_case(name, beam, dec, checker, flags=0):
  params, seqs, prefixes = _beam_data(name)
  del params
  ref = _beam_ref(name, beam)
  n_utt = len(seqs)
  plen = [len(p) for p in prefixes]
  state = {'first': True}

  def after(d, pos):
    out = d.stream_nbest(beam)
    assert (out['stable'] >= np.array(plen)).all(), (pos, out['stable'])
    lab, sc, _, status = d.stream_labels()
    assert status == 0
    for u in range(n_utt):
      live = int(out['counts'][u])
      assert np.array_equal(out['labels'][u][0][:pos[u]] if live else lab[u], lab[u]), u   # row 0 = stream_labels
      for k in range(live):
        assert np.array_equal(out['labels'][u][k][:plen[u]], prefixes[u]), (u, k)          # every labeling starts with the prefix
    if state['first']:   # directly after priming, nothing pushed
      state['first'] = False
      primed_u = [u for u in range(n_utt) if plen[u]]
      frames, offsets = oracle.pack([seqs[u][:plen[u]] for u in primed_u])
      want = checker.score_labels(frames, offsets, np.concatenate([prefixes[u] for u in primed_u]))
      for k, u in enumerate(primed_u):
        assert np.array_equal(lab[u], prefixes[u]), u
        assert int(out['counts'][u]) == 1, u
        assert _bits(sc[u]) == _bits(want[k]) == _bits(ref[u]['prefix_score']), u
        assert _bits(out['scores'][u][0]) == _bits(want[k]), u
      for u in range(n_utt):
        if not plen[u]:
          assert int(out['counts'][u]) == 0 and len(lab[u]) == 0 and sc[u] == 0.0, u

  rest = [len(s) - p for s, p in zip(seqs, plen)]
  schedule = _random_schedule(np.random.default_rng(beam), rest, 6)
  labels, scores, overflow, status, info, primed = _primed_stream(dec, seqs, prefixes, beam, schedule, 16, flags=flags, after=after)
  assert status == 0 and not overflow.any()
  for u in range(n_utt):
    assert _bits(primed[u]) == _bits(ref[u]['prefix_score'] if plen[u] else np.float32(0.0)), u
  _check_against_ref(ref, beam, labels, scores, info, (name, beam, flags))


@pytest.mark.parametrize('name', ['tracker_256_512', 'init_33_17_2'])
@pytest.mark.parametrize('beam', [6, 10])
def test_beam_search_from_a_primed_state(name, beam, oracle_lib):
  params = _beam_data(name)[0]
  dec, checker = _capi.Decoder(params), _capi.Decoder(params)
  _beam_case(name, beam, dec, checker)
  dec.close()
  checker.close()


# ---- 3. the reference's run from a primed BeamState

@pytest.mark.parametrize('case', ['trained_toy4', 'trained_d256', 'd20_h24_depth3'])
def test_the_reference_from_a_primed_state(case):
  data = np.load(os.path.join(golden_util.GOLDEN_DIR, 'fn_primed.npz'))
  params = weights.load_checkpoint(os.path.join(golden_util.GOLDEN_DIR, str(data[case + '/checkpoint'])))
  lengths = [int(n) for n in data[case + '/lengths']]
  plen = [int(n) for n in data[case + '/prefix_lengths']]
  beam = int(data['beam_size'])
  dim = int(params['observation_dim'])
  seqs = [synth.make_utterance(int(data[case + '/utt_seed']) + u, n, dim)[0] for u, n in enumerate(lengths)]
  bounds = np.concatenate([[0], np.cumsum(lengths)])
  dec = _capi.Decoder(params)
  for k in range(int(data[case + '/n_labelings'])):
    want = data['{}/labels_{}'.format(case, k)]
    want = [want[bounds[u]:bounds[u + 1]] for u in range(len(seqs))]
    prefixes = [w[:p] for w, p in zip(want, plen)]
    rest = [n - p for n, p in zip(lengths, plen)]
    labels, scores, overflow, status, _, primed = _primed_stream(dec, seqs, prefixes, beam, [rest], max(lengths))
    assert status == 0 and not overflow.any()
    for u in range(len(seqs)):
      assert np.array_equal(labels[u], want[u]), (case, k, u)
    np.testing.assert_allclose(scores, data['{}/scores_{}'.format(case, k)], rtol=1e-4)
    np.testing.assert_allclose(primed, data['{}/prefix_scores_{}'.format(case, k)], rtol=1e-4)
  dec.close()


# ---- 4. a persistent session

def test_priming_a_persistent_session(oracle_lib):
  """Four utterances primed, single-frame pushes through the mailbox, then a fifth (and the two after it) primed
  while the launch is resident, having received nothing: it leaves for the call, the next push starts a new one.
  On a whole MI355X the session must be accepted as a persistent one: a refusal fails the test."""
  if not gh._whole_device():   # pylint: disable=protected-access
    pytest.skip('not a whole MI355X')
  beam = 6
  params, seqs, prefixes = _beam_data('tracker_256_512')
  ref = _beam_ref('tracker_256_512', beam)
  n_utt = len(seqs)
  late = {4, 5, 6}   # (primed second; they receive nothing before)
  dec = _capi.Decoder(params)
  dec.stream_begin(n_utt, beam, 16, flags=_capi.UIS_FLAG_PERSISTENT)
  try:
    def prime(which):
      dec.stream_prime([seqs[u][:len(prefixes[u])] if u in which and len(prefixes[u]) else None for u in range(n_utt)],
                       [prefixes[u] if u in which and len(prefixes[u]) else None for u in range(n_utt)])

    def push_one(skip):
      chunks = []
      for u in range(n_utt):
        take = u not in skip and pos[u] < len(seqs[u])
        chunks.append(seqs[u][pos[u]:pos[u] + 1] if take else None)
        pos[u] += 1 if take else 0
      dec.stream_push(chunks)

    pos = [0] * n_utt
    prime({0, 1, 2, 3})
    for u in (0, 1, 2, 3):
      pos[u] = len(prefixes[u])
    for _ in range(3):
      push_one(late)
    prime(late)
    for u in late:
      pos[u] = len(prefixes[u])
    while any(pos[u] < len(seqs[u]) for u in range(n_utt)):
      push_one(())
    labels, scores, overflow, status = dec.stream_labels()
    assert status == 0 and not overflow.any()
    _check_against_ref(ref, beam, labels, scores, _info(dec, n_utt, beam), 'persistent')
  finally:
    dec.stream_end()
  dec.close()


def test_online_session_prime_in_a_persistent_session(oracle_lib):
  if not gh._whole_device():   # pylint: disable=protected-access
    pytest.skip('not a whole MI355X')
  beam = 6
  params, seqs, prefixes = _beam_data('tracker_256_512')
  ref = _beam_ref('tracker_256_512', beam)
  model_args, _, inference_args = uisrnn_amd.parse_arguments(['--observation_dim', '256', '--rnn_hidden_size', '512'])
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params)
  inference_args.beam_size, inference_args.look_ahead, inference_args.test_iteration = beam, 1, 1
  with model.online(len(seqs), inference_args, 16, persistent=True) as session:
    assert session.persistent   # (OnlineSession falls back to ordinary launches where the shape is refused: not here)
    names = 'abcdefgh'
    got = session.prime([s[:len(p)] if len(p) else None for s, p in zip(seqs, prefixes)],
                        [[names[c] for c in p] if len(p) else None for p in prefixes])
    for u, p in enumerate(prefixes):
      assert (got[u] is None) == (len(p) == 0)
      if len(p):
        assert _bits(got[u]) == _bits(ref[u]['prefix_score'])
    session.push([s[len(p):] for s, p in zip(seqs, prefixes)])
    labels = session.labels()
    for u, r in enumerate(ref):
      assert labels[u] == r['labels'][0].tolist(), u
    with pytest.raises(ValueError, match='already received'):
      session.prime([seqs[0][:2]] + [None] * (len(seqs) - 1), [[0, 0]] + [None] * (len(seqs) - 1))
    assert all(a >= len(p) for a, p in zip(session.stable_frames(), prefixes))


# ---- 5. refusals leave the session as it was

def test_refusals_leave_the_session_intact(oracle_lib):
  params = synth.tracker_params(256, 512, 1, seed=21)
  lens = [17, 45, 8]
  seqs, _ = synth.make_utterances(12_004, 3, lens, 256)
  beam, cap, max_frames = 4, 4, 50
  dec = _capi.Decoder(params)
  frames, offsets = oracle.pack(seqs)
  off = dec.decode(frames, offsets, beam, 1, 1, max_clusters=cap, want_beam_scores=True)
  assert off['status'] == 0 and not off['overflow'].any()
  m0, _ = dec.constants()
  bad_frame = seqs[1].copy()
  bad_frame[0, 0] = float(m0[0])   # weighted_mse's zero-first-difference quirk: frame 0 scores non-finite
  long_prefix = np.concatenate([seqs[1], seqs[1]])[:max_frames + 1]
  ok2 = (seqs[2][:2], np.array([0, 1], dtype=np.int32))   # a valid prefix in the same call: it must not be committed either
  refusals = [
      ('cluster cap', _capi.UIS_ERR_CLUSTER_CAP, 0, (seqs[0][:5], np.arange(5, dtype=np.int32)), 0),
      ('first appearance', _capi.UIS_ERR_INVALID_ARG, 0, (seqs[0][:2], np.array([0, 2], dtype=np.int32)), 0),
      ('negative', _capi.UIS_ERR_INVALID_ARG, 0, (seqs[0][:2], np.array([0, -1], dtype=np.int32)), 0),
      ('has frames', _capi.UIS_ERR_INVALID_ARG, 0, (seqs[0][:2], np.array([0, 0], dtype=np.int32)), 3),
      ('max_frames', _capi.UIS_ERR_INVALID_ARG, 1, (long_prefix, np.zeros(max_frames + 1, dtype=np.int32)), 0),
      ('non-finite', _capi.UIS_ERR_INVALID_ARG, 1, (bad_frame[:2], np.array([0, 0], dtype=np.int32)), 0),
  ]
  for what, status, u_bad, (chunk, labels), pushed_first in refusals:
    dec.stream_begin(3, beam, max_frames, max_clusters=cap)
    try:
      pos = [0, 0, 0]
      if pushed_first:
        dec.stream_push([seqs[0][:pushed_first], None, None])
        pos[0] = pushed_first
      chunks, labs = [None, None, ok2[0]], [None, None, ok2[1]]
      chunks[u_bad], labs[u_bad] = chunk, labels
      with pytest.raises(_capi.HipLibraryError) as err:
        dec.stream_prime(chunks, labs)
      assert err.value.status == status, what
      if what == 'non-finite':
        assert 'utterance 1' in str(err.value)
      dec.stream_push([s[p:] for s, p in zip(seqs, pos)])
      got, scores, overflow, rc = dec.stream_labels()
      assert rc == 0 and not overflow.any(), what
      for u in range(3):
        assert np.array_equal(got[u], off['labels'][offsets[u]:offsets[u + 1]]), (what, u)
      assert np.array_equal(_bits(scores), _bits(off['scores'])), what
      assert np.array_equal(_bits(_info(dec, 3, beam)), _bits(off['beam_scores'])), what
    finally:
      dec.stream_end()
  dec.close()


def test_a_prefix_may_fill_the_cluster_cap(oracle_lib):
  """K = max_clusters is accepted; the next new cluster flags the overflow as in any session."""
  params, seqs, ref, _ = _greedy('tracker_256_512')
  u = max(range(len(seqs)), key=lambda k: int(ref['max_clusters'][k]))
  labels = ref['labels'][u]
  assert int(labels.max()) >= 2
  p2 = int(np.argmax(labels == 2))   # the frame that opens the third cluster
  dec = _capi.Decoder(params)
  dec.stream_begin(1, 1, len(labels), max_clusters=2)
  try:
    dec.stream_prime([seqs[u][:p2]], [labels[:p2]])
    got, _, overflow, rc = dec.stream_labels()
    assert rc == 0 and not overflow.any() and np.array_equal(got[0], labels[:p2])
    dec.stream_push([seqs[u][p2:]])
    _, _, overflow, rc = dec.stream_labels()
    assert rc == _capi.UIS_ERR_CLUSTER_CAP and overflow[0] == 1
  finally:
    dec.stream_end()
  dec.stream_begin(1, 1, len(labels), max_clusters=2)
  try:
    with pytest.raises(_capi.HipLibraryError) as err:
      dec.stream_prime([seqs[u][:p2 + 1]], [labels[:p2 + 1]])
    assert err.value.status == _capi.UIS_ERR_CLUSTER_CAP
  finally:
    dec.stream_end()
  dec.close()


# ---- 6. stale memory

@pytest.mark.parametrize('word', WORDS)
def test_no_output_depends_on_stale_memory(word, oracle_lib, monkeypatch):
  _env(monkeypatch, word)
  params = _greedy('init_33_17_2')[0]
  dec = _capi.Decoder(params)
  _greedy_case('init_33_17_2', dec, (_capi.UIS_FLAG_STEPWISE, 0), rng_seed=3)
  dec.close()
  params = _beam_data('tracker_256_512')[0]
  dec, checker = _capi.Decoder(params), _capi.Decoder(params)
  _beam_case('tracker_256_512', 6, dec, checker)
  _beam_case('tracker_256_512', 6, dec, checker, flags=_capi.UIS_FLAG_STEPWISE)
  dec.close()
  checker.close()


# ---- 7. the Python layer

def test_predict_primed(oracle_lib):
  beam = 6
  params, seqs, prefixes = _beam_data('tracker_256_512')
  ref = _beam_ref('tracker_256_512', beam)
  model_args, _, inference_args = uisrnn_amd.parse_arguments(['--observation_dim', '256', '--rnn_hidden_size', '512'])
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params)
  inference_args.beam_size, inference_args.look_ahead, inference_args.test_iteration = beam, 1, 1
  names = ['spk_a', 'spk_b', 'spk_c']
  got = model.predict_primed(seqs, [[names[c] for c in p] for p in prefixes], inference_args)
  for u, r in enumerate(ref):
    assert got[u] == r['labels'][0].tolist(), u
  assert model.predict_primed(seqs[0], prefixes[0].tolist(), inference_args) == ref[0]['labels'][0].tolist()
  # an empty prefix: predict
  assert model.predict_primed(seqs, [[] for _ in seqs], inference_args) == model.predict(seqs, inference_args)
  assert model.predict_primed(seqs[1], [], inference_args) == model.predict(seqs[1], inference_args)


def _greedy_model(beam, max_clusters):
  params = _greedy('tracker_256_512')[0]
  model_args, _, inference_args = uisrnn_amd.parse_arguments(['--observation_dim', '256', '--rnn_hidden_size', '512'])
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params)
  inference_args.beam_size, inference_args.look_ahead, inference_args.test_iteration = beam, 1, 1
  inference_args.max_clusters = max_clusters
  return model, inference_args


def test_predict_primed_doubles_the_cluster_cap(oracle_lib, monkeypatch):
  """args.max_clusters 2: a prefix with three clusters is refused by uis_stream_prime (UIS_ERR_CLUSTER_CAP), a prefix
  with two is accepted and the continuation overflows; either way the batch is reopened with twice the cap until it
  fits, and the answer is the unconstrained decode's."""
  _, seqs, ref, _ = _greedy('tracker_256_512')
  u = max(range(len(seqs)), key=lambda k: int(ref['max_clusters'][k]))
  labels = ref['labels'][u]
  assert int(ref['max_clusters'][u]) >= 3
  p2 = int(np.argmax(labels == 2))   # the frame that opens the third cluster
  model, inference_args = _greedy_model(1, 2)
  decoder = model._get_decoder()   # pylint: disable=protected-access
  caps, begin = [], decoder.stream_begin

  def spy(n_utt, beam_size, max_frames, max_clusters=0, flags=0):
    caps.append(max_clusters)
    return begin(n_utt, beam_size, max_frames, max_clusters=max_clusters, flags=flags)

  monkeypatch.setattr(decoder, 'stream_begin', spy)
  fits = [c for c in (2, 4, 8, 16) if c < 2 * int(ref['max_clusters'][u])]   # (the caps tried: up to the first that holds K)
  assert model.predict_primed(seqs[u], labels[:p2 + 1].tolist(), inference_args) == labels.tolist()
  assert caps == fits and len(caps) >= 2, caps       # (the first refusal came from the prefix itself)
  del caps[:]
  assert model.predict_primed(seqs[u], labels[:p2].tolist(), inference_args) == labels.tolist()
  assert caps == fits, caps                          # (... and here from the overflow flag after the push)
  # in a list: only the flagged utterance is decoded again
  short = min(range(len(seqs)), key=lambda k: (int(ref['max_clusters'][k]), -len(seqs[k])))
  assert int(ref['max_clusters'][short]) <= 2
  del caps[:]
  got = model.predict_primed([seqs[short], seqs[u]], [[], labels[:p2].tolist()], inference_args)
  assert got == [ref['labels'][short].tolist(), labels.tolist()] and caps == fits


def test_predict_primed_raises_for_an_emptied_beam(oracle_lib):
  """A frame of NaNs behind the prefix: every candidate is non-finite, no hypothesis survives."""
  _, seqs, ref, _ = _greedy('tracker_256_512')
  seq = seqs[0][:12].copy()
  seq[6] = np.nan
  model, inference_args = _greedy_model(4, 0)
  with pytest.raises(uisrnn_amd.EmptyBeamError):
    model.predict_primed(seq, ref['labels'][0][:5].tolist(), inference_args)
  with pytest.raises(uisrnn_amd.EmptyBeamError):
    model.predict_primed([seqs[1], seq], [[], ref['labels'][0][:5].tolist()], inference_args)
  assert model.predict_primed(seqs[0][:12], ref['labels'][0][:5].tolist(), inference_args)[:5] == ref['labels'][0][:5].tolist()
