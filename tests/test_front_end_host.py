"""The Python front end's plumbing, pinned with stand-in decoders: no device, no library.

What uisrnn_amd/uisrnn.py does around the library calls -- regrouping a batch (cap retry, halves after UIS_ERR_OOM,
look-ahead retry groups) with every utterance's own max_speakers entry and transition_bias table, the one decode
request behind the five offline entry points, which bad argument is reported first, predict_primed's cap loop and
the halving of score_labels / score_speakers.  The expected values were recorded before the front end was
consolidated and hold on both sides of that change.
"""

import numpy as np
import pytest

import uisrnn_amd
from uisrnn_amd import _capi
from uisrnn_amd import arguments

DIM = 4


def _model(**inference):
  model_args, _, inference_args = arguments.parse_arguments([])
  model_args.observation_dim = DIM
  for key, value in inference.items():
    setattr(inference_args, key, value)
  return uisrnn_amd.UISRNN(model_args), inference_args


def _error(status, text):
  err = _capi.HipLibraryError('stand-in failed ({}): {}'.format(status, text))
  err.status = status
  return err


def _tagged(n_utt, need=()):
  """Utterance k: 3 + k % 4 frames, k in column 0, the level capacity it needs in column 1."""
  seqs = []
  for k in range(n_utt):
    s = np.zeros((3 + k % 4, DIM))
    s[:, 0] = k
    s[:, 1] = need[k] if k < len(need) else 100
    seqs.append(s)
  return seqs


# ---- 1. regrouping keeps each utterance's own tables

class _Regrouped:
  """decode_f64 that checks the tables it is handed against the tags of the sequences it is handed; at most `room`
  utterances per call; utterance k needs a level capacity of its column 1."""

  def __init__(self, room=99, tables=True):
    self.room, self.tables, self.calls, self.flags = room, tables, [], np.zeros(0, dtype=np.int32)

  def decode_f64(self, seqs, beam_size, look_ahead, test_iteration, max_clusters=0, flags=0, level_cap=0, **tables):
    cap = level_cap or 32768
    tags = [int(s[0, 0]) for s in seqs]
    self.calls.append((tags, cap))
    if not self.tables:
      assert not tables, sorted(tables)   # (no limits, no bias: not even as a keyword)
    else:
      assert sorted(tables) == ['bias', 'limits']
      assert list(tables['limits']) == [t + 1 for t in tags]
      assert tables['bias'].shape == (sum(s.shape[0] for s in seqs),)
      at = 0
      for s, t in zip(seqs, tags):
        assert (tables['bias'][at:at + s.shape[0]] == (t + 1) / 16).all(), (t, tables['bias'][at:at + s.shape[0]])
        at += s.shape[0]
    if len(seqs) > self.room:
      self.flags = np.zeros(0, dtype=np.int32)
      raise _error(_capi.UIS_ERR_OOM, 'decode state would need 999 GB')
    self.flags = np.array([2 if int(s[0, 1]) > cap else 0 for s in seqs], dtype=np.int32)
    if self.flags.any():
      raise _error(_capi.UIS_ERR_UNSUPPORTED, 'a look-ahead window held more prefixes than a level')
    labels = np.concatenate([np.full(s.shape[0], t, dtype=np.int32) for s, t in zip(seqs, tags)])
    return {'status': 0, 'labels': labels, 'overflow': np.zeros(len(seqs), dtype=np.int32),
            'stats': {'decode_kernel': 'stand-in'}}

  def last_overflow(self, n_utt=None):
    return self.flags


_NEED = [100, 40000, 100, 300000, 100, 100, 9_000_000, 100]   # (tests/test_host_api.py: the look-ahead retry's)


def _tables(seqs):
  return ([k + 1 for k in range(len(seqs))],
          [np.full(s.shape[0], (k + 1) / 16) for k, s in enumerate(seqs)])


def test_halves_after_oom_carry_each_utterances_own_limits_and_bias():
  model, args = _model()
  seqs = _tagged(11)
  limits, bias = _tables(seqs)
  dec = _Regrouped(room=3)
  out = model._decode_batch(seqs, args, decoder=dec, limits=limits, bias=bias)  # pylint: disable=protected-access
  assert out == [[k] * s.shape[0] for k, s in enumerate(seqs)]
  done = [tags for tags, _ in dec.calls if len(tags) <= 3]
  assert sorted(t for tags in done for t in tags) == list(range(11))
  assert dec.calls[0][0] == list(range(11)) and dec.calls[1][0] == list(range(0, 11, 2))   # (alternating halves)


@pytest.mark.parametrize('room', [99, 3])
def test_look_ahead_retry_groups_carry_each_utterances_own_limits_and_bias(room):
  model, args = _model(look_ahead=3)
  seqs = _tagged(11, _NEED)
  limits, bias = _tables(seqs)
  dec = _Regrouped(room=room)
  with pytest.raises(uisrnn_amd.LookAheadWindowError) as info:
    model._decode_batch(seqs, args, decoder=dec, limits=limits, bias=bias)  # pylint: disable=protected-access
  assert info.value.utterances == (6,)
  assert info.value.status == _capi.UIS_ERR_UNSUPPORTED
  assert str(info.value).endswith('(utterances [6])') and str(info.value).count('(utterances') == 1
  assert info.value.results == [None if k == 6 else [k] * s.shape[0] for k, s in enumerate(seqs)]
  assert sorted({cap for _, cap in dec.calls}) == [32768, 262144, 524287]
  # without the hopeless one: every utterance, in the caller's order
  keep = [k for k in range(11) if k != 6]
  dec = _Regrouped(room=room)
  out = model._decode_batch([seqs[k] for k in keep], args, decoder=dec,  # pylint: disable=protected-access
                            limits=[limits[k] for k in keep], bias=[bias[k] for k in keep])
  assert out == [[k] * seqs[k].shape[0] for k in keep]


@pytest.mark.parametrize('room,look_ahead', [(3, 1), (99, 3)])
def test_without_tables_the_decoder_receives_neither_keyword(room, look_ahead):
  model, args = _model(look_ahead=look_ahead)
  seqs = _tagged(6, _NEED if look_ahead > 1 else ())
  dec = _Regrouped(room=room, tables=False)
  out = model._decode_batch(seqs, args, decoder=dec)  # pylint: disable=protected-access
  assert out == [[k] * s.shape[0] for k, s in enumerate(seqs)]
  assert len(dec.calls) > 1


# ---- 2. the five offline entry points request the same decode

class _Recorder:
  """Records what decode_f64 is asked; answers label 0 everywhere, two hypotheses, confidence 0.5."""

  def __init__(self):
    self.requests, self.lens = [], []

  def decode_f64(self, seqs, beam_size, look_ahead, test_iteration, max_clusters=0, flags=0, level_cap=0,
                 limits=None, bias=None):
    self.lens = [s.shape[0] for s in seqs]
    self.requests.append({'seqs': [id(s) for s in seqs], 'opts': (beam_size, look_ahead, test_iteration),
                          'limits': None if limits is None else list(limits),
                          'bias': None if bias is None else np.asarray(bias).tolist(),
                          'max_clusters': max_clusters, 'flags': flags, 'level_cap': level_cap})
    return {'status': 0, 'labels': np.zeros(sum(self.lens), dtype=np.int32),
            'overflow': np.zeros(len(seqs), dtype=np.int32), 'stats': {}}

  def last_nbest(self, n_best):
    return {'labels': [np.zeros((n_best, n), dtype=np.int32) for n in self.lens],
            'scores': np.tile(np.arange(n_best, dtype=np.float32), (len(self.lens), 1)),
            'counts': np.full(len(self.lens), min(n_best, 2), dtype=np.int32)}

  def last_posterior(self, temperature):
    return {'confidence': [np.full(n, 0.5, dtype=np.float32) for n in self.lens],
            'change': [np.zeros(n, dtype=np.float32) for n in self.lens]}


def _recorded(call):
  model, args = _model()
  rec = _Recorder()
  model._get_decoder = lambda device=None: rec  # pylint: disable=protected-access
  out = call(model, args)
  assert len(rec.requests) == 1
  return out, rec.requests[0]


def test_offline_entry_points_request_the_same_decode_for_an_array():
  seq = np.random.RandomState(0).rand(5, DIM)
  kw = dict(max_speakers=3, transition_bias=np.array([0.5, 0.25, np.nan, 1.0, 0.0]))
  labels, want = _recorded(lambda m, a: m.predict(seq, a, **kw))
  assert labels == [0] * 5
  assert want['seqs'] == [id(seq)] and want['limits'] == [3] and want['max_clusters'] == 16
  assert want['flags'] == 0 and want['level_cap'] == 0 and want['opts'] == (10, 1, 2)
  np.testing.assert_equal(want['bias'], [0.5, 0.25, np.nan, 1.0, 0.0])
  single, req = _recorded(lambda m, a: m.predict_single(seq, a, **kw))
  assert single == labels and repr(req) == repr(want)
  pair, req = _recorded(lambda m, a: m.predict_nbest(seq, a, n_best=4, **kw))
  assert repr(req) == repr(want)
  assert isinstance(pair, tuple) and pair == ([[0] * 5, [0] * 5], [0.0, 1.0])
  triple, req = _recorded(lambda m, a: m.predict_posteriors(seq, a, temperature=2.0, **kw))
  assert repr(req) == repr(want)
  assert isinstance(triple, tuple) and len(triple) == 3 and triple[0] == labels
  assert triple[1].tolist() == [0.5] * 5 and triple[2].tolist() == [0.0] * 5


def test_offline_entry_points_request_the_same_decode_for_a_list():
  rng = np.random.RandomState(1)
  seqs = [rng.rand(n, DIM) for n in (4, 2, 3)]
  kw = dict(max_speakers=[2, 0, 5], transition_bias=[np.full(4, 0.5), None, [1.0, 0.0, 0.25]])
  labels, want = _recorded(lambda m, a: m.predict(seqs, a, **kw))
  assert labels == [[0] * 4, [0] * 2, [0] * 3]
  assert want['seqs'] == [id(s) for s in seqs] and want['limits'] == [2, 0, 5] and want['max_clusters'] == 16
  assert want['flags'] == 0 and want['level_cap'] == 0
  np.testing.assert_equal(want['bias'], [0.5] * 4 + [np.nan] * 2 + [1.0, 0.0, 0.25])
  par, req = _recorded(lambda m, a: uisrnn_amd.parallel_predict(m, seqs, a, devices=[0], **kw))
  assert par == labels and repr(req) == repr(want)
  pairs, req = _recorded(lambda m, a: m.predict_nbest(seqs, a, **kw))
  assert repr(req) == repr(want)
  assert pairs == [([[0] * n, [0] * n], [0.0, 1.0]) for n in (4, 2, 3)]
  triples, req = _recorded(lambda m, a: m.predict_posteriors(seqs, a, **kw))
  assert repr(req) == repr(want)
  assert [t[0] for t in triples] == labels and [t[1].shape for t in triples] == [(4,), (2,), (3,)]
  assert all(isinstance(t, tuple) and len(t) == 3 for t in triples)


def test_offline_entry_points_answer_an_empty_list_without_a_decoder():
  model, args = _model()

  def no_device(device=None):
    raise AssertionError('an empty list needs no decoder')
  model._get_decoder = no_device  # pylint: disable=protected-access
  assert model.predict([], args) == []
  assert model.predict_nbest([], args) == []
  assert model.predict_posteriors([], args) == []
  assert uisrnn_amd.parallel_predict(model, [], args, devices=[0]) == []
  assert model.predict_primed([], [], _model(test_iteration=1)[1]) == []


# ---- 3. which bad argument is reported

_GOOD = np.zeros((3, DIM))
_F32 = np.zeros((3, DIM), dtype=np.float32)        # a bad sequence dtype
_SEQ = 'test_sequence should be a numpy array of float type.'
_KIND = 'test_sequences should be either a list or numpy array.'
_SPEAKERS = 'max_speakers must be in [0, 4096], not -1.'
_BIAS = 'transition_bias of utterance 0 is 2.0 at frame 0: a value must be in [0, 1] or NaN.'
_NBEST = 'n_best must be in [1, args.beam_size = 10].'
_TEMP = 'temperature must be a finite number > 0, not 0.'
_IDS = [0, 0, 1]

# (entry point, positional arguments after the model, keywords, exception, message)
_PRECEDENCE = [
    # a bad sequence dtype with a bad max_speakers: an array's checks begin with the sequence, a list's with the bound
    ('predict', (_F32,), dict(max_speakers=-1), TypeError, _SEQ),
    ('predict', ([_GOOD, _F32],), dict(max_speakers=-1), ValueError, _SPEAKERS),
    ('predict_single', (_F32,), dict(max_speakers=-1), TypeError, _SEQ),
    ('predict_single', ([_GOOD],), dict(max_speakers=-1), TypeError, _SEQ),
    ('predict_nbest', (_F32,), dict(max_speakers=-1), TypeError, _SEQ),
    ('predict_nbest', ([_GOOD, _F32],), dict(max_speakers=-1), ValueError, _SPEAKERS),
    ('predict_posteriors', (_F32,), dict(max_speakers=-1), TypeError, _SEQ),
    ('predict_posteriors', ([_GOOD, _F32],), dict(max_speakers=-1), ValueError, _SPEAKERS),
    ('predict_primed', (_F32, [0]), dict(max_speakers=-1), ValueError, _SPEAKERS),
    ('predict_primed', ([_GOOD, _F32], [[0], []]), dict(max_speakers=-1), ValueError, _SPEAKERS),
    ('parallel_predict', ([_GOOD, _F32],), dict(max_speakers=-1, devices=[0]), TypeError, _SEQ),
    # a bad max_speakers with a bad transition_bias
    ('predict', (_GOOD,), dict(max_speakers=-1, transition_bias=2.0), ValueError, _SPEAKERS),
    ('predict', ([_GOOD],), dict(max_speakers=-1, transition_bias=2.0), ValueError, _SPEAKERS),
    ('predict_nbest', (_GOOD,), dict(max_speakers=-1, transition_bias=2.0), ValueError, _SPEAKERS),
    ('predict_nbest', ([_GOOD],), dict(max_speakers=-1, transition_bias=2.0), ValueError, _SPEAKERS),
    ('predict_posteriors', (_GOOD,), dict(max_speakers=-1, transition_bias=2.0), ValueError, _SPEAKERS),
    ('predict_posteriors', ([_GOOD],), dict(max_speakers=-1, transition_bias=2.0), ValueError, _SPEAKERS),
    ('parallel_predict', ([_GOOD],), dict(max_speakers=-1, transition_bias=2.0, devices=[0]), ValueError, _SPEAKERS),
    # a bad sequence with a bad transition_bias
    ('predict', (_F32,), dict(transition_bias=2.0), TypeError, _SEQ),
    ('predict', ([_F32],), dict(transition_bias=2.0), TypeError, _SEQ),
    ('score_labels', (_F32, _IDS), dict(transition_bias=2.0), TypeError, _SEQ),
    ('score_labels', ([_GOOD, _F32], [_IDS, _IDS]), dict(transition_bias=2.0), TypeError, _SEQ),
    ('score_speakers', (_F32, _IDS), dict(transition_bias=2.0), TypeError, _SEQ),
    ('score_speakers', ([_GOOD, _F32], [_IDS, _IDS]), dict(transition_bias=2.0), TypeError, _SEQ),
    ('score_labels', (_GOOD, _IDS[:2]), dict(transition_bias=2.0), ValueError,
     'test_cluster_ids has 2 ids for a sequence of 3 frames.'),
    ('score_speakers', ([_GOOD], [_IDS]), dict(transition_bias=2.0), ValueError, _BIAS),
    # a bad n_best or temperature with a bad sequence
    ('predict_nbest', (_F32,), dict(n_best=0), ValueError, _NBEST),
    ('predict_nbest', ([_F32],), dict(n_best=0), ValueError, _NBEST),
    ('predict_nbest', ((_GOOD,),), dict(n_best=True), ValueError, 'n_best must be an integer in [1, args.beam_size].'),
    ('predict_posteriors', (_F32,), dict(temperature=0), ValueError, _TEMP),
    ('predict_posteriors', ([_F32],), dict(temperature=0), ValueError, _TEMP),
    ('predict_posteriors', ((_GOOD,),), dict(temperature=0), ValueError, _TEMP),
    # a non-list input with anything else
    ('predict', ((_F32,),), dict(max_speakers=-1, transition_bias=2.0), TypeError, _KIND),
    ('predict_nbest', ((_F32,),), dict(max_speakers=-1), TypeError, _KIND),
    ('predict_posteriors', ((_F32,),), dict(transition_bias=2.0), TypeError, _KIND),
    ('predict_primed', ((_F32,), [[0]]), dict(max_speakers=-1), TypeError, _KIND),
    ('predict_primed', ([_GOOD, _F32], [[0]]), dict(max_speakers=-1), ValueError,
     'prefix_cluster_ids must be a list with one id sequence per test sequence.'),
    ('score_labels', ((_F32,), [_IDS]), dict(transition_bias=2.0), TypeError, _KIND),
    ('score_speakers', ((_F32,), [_IDS]), dict(transition_bias=2.0), TypeError, _KIND),
    ('score_labels', ([_F32], _IDS), dict(transition_bias=2.0), ValueError,
     'test_cluster_ids must be a list with one id sequence per test sequence.'),
    ('parallel_predict', (_GOOD,), dict(max_speakers=-1, devices=[0]), TypeError, 'test_sequences must be a list.'),
    ('parallel_predict', ((_GOOD,),), dict(transition_bias=2.0, devices=[0]), TypeError, 'test_sequences must be a list.'),
]


@pytest.mark.parametrize('row', range(len(_PRECEDENCE)))
def test_which_bad_argument_is_reported(row):
  name, positional, keywords, kind, message = _PRECEDENCE[row]
  model, args = _model(test_iteration=1 if name == 'predict_primed' else 2)

  def no_device(device=None):
    raise AssertionError('a refused argument must not reach the device')
  model._get_decoder = no_device  # pylint: disable=protected-access
  with pytest.raises((TypeError, ValueError)) as info:
    if name == 'parallel_predict':
      uisrnn_amd.parallel_predict(model, positional[0], args, **keywords)
    elif name.startswith('score_'):
      getattr(model, name)(*positional, **keywords)
    elif name == 'predict_primed':
      model.predict_primed(positional[0], positional[1], args, **keywords)
    else:
      getattr(model, name)(positional[0], args, **keywords)
  assert type(info.value) is kind and str(info.value) == message, (name, info.value)


# ---- 4. predict_primed's cap loop

class _PrimedSession:
  """stream_prime refuses (UIS_ERR_CLUSTER_CAP) below 32 clusters; utterance k (column 0 of its prefix) overflows
  below the cap in its column 1; labels are the accepting attempt's cap."""

  def __init__(self, refuse=None):
    self.refuse, self.begun, self.ended, self.caps, self.limits, self.members = refuse, 0, 0, [], [], []

  def stream_begin(self, n_utt, beam_size, max_frames, max_clusters=0, flags=0, limits=None):
    assert self.begun == self.ended
    self.begun += 1
    self.cap, self.n_utt = max_clusters, n_utt
    self.caps.append(max_clusters)
    self.limits.append(limits)

  def stream_prime(self, chunks, labels):
    assert len(chunks) == len(labels) == self.n_utt
    assert all(lab.dtype == np.int32 and len(lab) == len(c) for c, lab in zip(chunks, labels))
    self.tags = [int(c[0, 0]) for c in chunks]
    self.need = [int(c[0, 1]) for c in chunks]
    self.have = [len(c) for c in chunks]
    self.prefix = [lab.tolist() for lab in labels]
    self.members.append(self.tags)
    if self.refuse is not None:
      raise _error(self.refuse, 'refused')
    if self.cap < 32:
      raise _error(_capi.UIS_ERR_CLUSTER_CAP, 'a prefix with more clusters than the tables hold')

  def stream_push(self, chunks):
    assert len(chunks) == self.n_utt
    self.have = [h + (0 if c is None else len(c)) for h, c in zip(self.have, chunks)]

  def stream_labels(self):
    overflow = np.array([1 if need > self.cap else 0 for need in self.need], dtype=np.int32)
    per_utt = [np.array(p + [self.cap] * (h - len(p)), dtype=np.int32) for p, h in zip(self.prefix, self.have)]
    return per_utt, np.zeros(self.n_utt, dtype=np.float32), overflow, 0

  def stream_end(self):
    self.ended += 1


def _primed(need, refuse=None, **keywords):
  model, args = _model(test_iteration=1)
  dec = _PrimedSession(refuse)
  model._get_decoder = lambda device=None: dec  # pylint: disable=protected-access
  seqs = _tagged(len(need), need)
  prefixes = [['b', 'a', 'b'][:1 + k % 3] for k in range(len(need))]
  return model, dec, lambda: model.predict_primed(seqs, prefixes, args, **keywords)


def test_predict_primed_doubles_the_cap_and_keeps_the_survivors_labels():
  _, dec, run = _primed([1, 1, 64, 1], max_speakers=[1, 2, 3, 4])
  out = run()
  assert dec.caps == [16, 32, 64] and dec.members == [[0, 1, 2, 3], [0, 1, 2, 3], [2]]
  assert dec.limits == [[1, 2, 3, 4], [1, 2, 3, 4], [3]]       # (each retry's bounds are its members')
  assert dec.begun == dec.ended == 3
  # the renamed prefix, then the cap of the attempt that accepted the utterance
  assert out == [[0, 32, 32], [0, 1, 32, 32], [0, 1, 0, 64, 64], [0, 32, 32, 32, 32, 32]]
  _, dec, run = _primed([1, 64])
  assert run() == [[0, 32, 32], [0, 1, 64, 64]] and dec.limits == [None, None, None]


def test_predict_primed_gives_up_beyond_the_librarys_cluster_limit():
  _, dec, run = _primed([1, 10000])
  with pytest.raises(RuntimeError) as info:
    run()
  assert str(info.value) == 'more than 4096 clusters per hypothesis'
  assert dec.caps == [16, 32, 64, 128, 256, 512, 1024, 2048, 4096] and dec.begun == dec.ended == 9


def test_predict_primed_ends_the_session_when_the_prime_is_refused():
  _, dec, run = _primed([1, 1], refuse=_capi.UIS_ERR_INVALID_ARG)
  with pytest.raises(_capi.HipLibraryError) as info:
    run()
  assert info.value.status == _capi.UIS_ERR_INVALID_ARG and dec.caps == [16] and dec.begun == dec.ended == 1


# ---- 5. score_labels / score_speakers in halves

class _Scorer:
  """At most `room` utterances per call.  An utterance's score is its tag (column 0; -1 without frames), a frame's
  loss tag + 0.25, row t of the speakers' losses 100 * tag + the column."""

  def __init__(self, room, tables):
    self.room, self.tables, self.calls = room, tables, []

  def _tags(self, frames, offsets, labels, bias):
    assert frames.dtype == np.float32 and labels.dtype == np.int32 and labels.shape == (frames.shape[0],)
    assert int(offsets[-1]) == frames.shape[0]
    tags = [int(frames[a, 0]) if b > a else -1 for a, b in zip(offsets[:-1], offsets[1:])]
    self.calls.append(tags)
    if self.tables:
      assert bias.shape == (frames.shape[0],) and (bias == (frames[:, 0] + 1) / 16).all()
    else:
      assert bias is None
    if len(tags) > self.room:
      raise _error(_capi.UIS_ERR_OOM, 'does not fit')
    return tags

  def score_labels(self, frames, offsets, labels, want_frame_losses=False, bias=None):
    tags = self._tags(frames, offsets, labels, bias)
    assert want_frame_losses
    return np.array(tags, dtype=np.float32), frames[:, 0] + np.float32(0.25)

  def score_speakers(self, frames, offsets, labels, width, bias=None):
    tags = self._tags(frames, offsets, labels, bias)
    assert width == max(int(labels[a:b].max()) + 2 if b > a else 1 for a, b in zip(offsets[:-1], offsets[1:]))
    return None, (100 * frames[:, :1] + np.arange(width, dtype=np.float32)).astype(np.float32)


def _scored(room, tables=True):
  model, _ = _model()
  dec = _Scorer(room, tables)
  model._get_decoder = lambda device=None: dec  # pylint: disable=protected-access
  seqs = [np.full((n, DIM), float(k)) for k, n in enumerate((3, 4, 0, 2, 5))]
  ids = [[('s', t % (k + 1)) for t in range(s.shape[0])] for k, s in enumerate(seqs)]
  bias = [np.full(s.shape[0], (k + 1) / 16) for k, s in enumerate(seqs)] if tables else None
  return model, dec, seqs, ids, bias


@pytest.mark.parametrize('tables', [True, False])
def test_score_labels_in_halves_keeps_order_losses_and_bias(tables):
  model, dec, seqs, ids, bias = _scored(2, tables)
  scores, losses = model.score_labels(seqs, ids, per_frame=True, transition_bias=bias)
  assert scores == [0.0, 1.0, -1.0, 3.0, 4.0] and all(isinstance(x, float) for x in scores)
  assert [x.tolist() for x in losses] == [[k + 0.25] * s.shape[0] for k, s in enumerate(seqs)]
  assert all(x.dtype == np.float32 for x in losses)
  assert dec.calls == [[0, 1, -1, 3, 4], [0, -1, 4], [0, 4], [-1], [1, 3]]
  assert model.score_labels(seqs, ids, transition_bias=bias) == scores
  # one array: a float, or the pair with its losses
  one = model.score_labels(seqs[3], ids[3], transition_bias=None if bias is None else bias[3])
  assert isinstance(one, float) and one == 3.0
  one, its = model.score_labels(seqs[3], ids[3], per_frame=True, transition_bias=None if bias is None else bias[3])
  assert one == 3.0 and its.tolist() == [3.25, 3.25]
  assert model.score_labels([], []) == [] and model.score_labels([], [], per_frame=True) == ([], [])


@pytest.mark.parametrize('tables', [True, False])
def test_score_speakers_in_halves_cuts_each_utterances_own_width(tables):
  model, dec, seqs, ids, bias = _scored(2, tables)
  out = model.score_speakers(seqs, ids, transition_bias=bias)
  widths = [2, 3, 1, 3, 6]   # (speakers + 1; 1 without frames)
  assert [x.shape for x in out] == [(s.shape[0], w) for s, w in zip(seqs, widths)]
  for k, (x, w) in enumerate(zip(out, widths)):
    assert x.dtype == np.float32 and (x == 100 * k + np.arange(w)).all()
  assert dec.calls == [[0, 1, -1, 3, 4], [0, -1, 4], [0, 4], [-1], [1, 3]]
  one = model.score_speakers(seqs[4], ids[4], transition_bias=None if bias is None else bias[4])
  assert one.shape == (5, 6) and (one == 400 + np.arange(6)).all()
  assert model.score_speakers([], []) == []


def test_a_single_utterance_that_does_not_fit_is_an_error_not_a_loop():
  model, dec, seqs, ids, _ = _scored(0, tables=False)
  with pytest.raises(_capi.HipLibraryError) as info:
    model.score_labels(seqs[:1], ids[:1])
  assert info.value.status == _capi.UIS_ERR_OOM and dec.calls == [[0]]
  with pytest.raises(_capi.HipLibraryError):
    model.score_speakers(seqs[0], ids[0])
  assert dec.calls == [[0], [0]]
