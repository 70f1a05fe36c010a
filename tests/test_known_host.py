"""Known speakers on the CPU: the reference the GPU tests compare with, and the surface.

tests/known_ref.py restates the beam search with one tag per frame and a binding of tags to clusters beside each
hypothesis, on tests/limit_ref.py's walk.  With no table and with an all-zero table it is oracle.decode bit for bit,
with every frame tagged it is the forced labeling at forced_ref's score, with a tagged prefix it is the primed decode:
that is what makes it a reference.  The properties (equal tags, equal labels; different tags, different labels) are
read off the labels alone.  Then the keyword's checks and the regroupings of the Python front end, with the library
stubbed as tests/test_front_end_host.py does.  No GPU needed.
"""

import os
import re
import types

import numpy as np
import pytest

import forced_ref
import golden_util
import known_ref
import limit_ref
import uisrnn_amd
from uisrnn_amd import _capi
from uisrnn_amd import arguments
from uisrnn_amd import uisrnn as host

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM = 4


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _short(case, n_utt=2, frames=10):
  return [s[:frames] for s in case['seqs'][:n_utt]]


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2', 'd20_h24_depth3'])
@pytest.mark.parametrize('look_ahead', [1, 2, 3])
@pytest.mark.parametrize('test_iteration', [1, 2])
def test_without_tags_it_is_the_oracle_decode(name, look_ahead, test_iteration, oracle_lib):
  case = golden_util.load_case(name)
  seqs = _short(case, 2, 10 if look_ahead < 3 else 7) + [case['seqs'][-1][:1]]
  beam = 4 if look_ahead < 3 else 3
  ref = oracle_lib.decode(case['params'], seqs, beam, look_ahead, test_iteration, n_threads=2)
  for what, tags in (('no table', None), ('all zero', [np.zeros(len(s), dtype=np.uint8) for s in seqs])):
    got = known_ref.decode_list(case['params'], seqs, beam, look_ahead, test_iteration, tags=tags)
    for u in range(len(seqs)):
      assert np.array_equal(got['labels'][u], ref['labels'][u]), (what, u)
    assert np.array_equal(_bits(got['scores']), _bits(ref['scores'])), what
    assert np.array_equal(_bits(got['beam_scores']), _bits(ref['beam_scores'])), what
    assert np.array_equal(got['max_clusters'], ref['max_clusters']), what


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2'])
@pytest.mark.parametrize('look_ahead', [1, 2, 3])
def test_every_frame_tagged_is_the_forced_labeling(name, look_ahead, oracle_lib):
  case = golden_util.load_case(name)
  seq = case['seqs'][0][:11]
  tags = np.array([5, 5, 127, 5, 1, 1, 127, 9, 9, 5, 1], dtype=np.uint8)
  want = known_ref.first_appearance(tags)
  assert want.tolist() == [0, 0, 1, 0, 2, 2, 1, 3, 3, 0, 2]
  got = known_ref.decode(case['params'], seq, 4, look_ahead, 1, tags=tags)
  assert len(got['beam']) == 1 and got['labels'].tolist() == want.tolist()
  score, _ = forced_ref.score_one(case['params'], seq, want)
  assert _bits(got['score']) == _bits(score)
  # the second pass of test_iteration 2 is forced too, and lands on the same labels
  got = known_ref.decode(case['params'], seq, 4, look_ahead, 2, tags=tags)
  assert len(got['beam']) == 1 and got['beam'][0].trace == want.tolist() * 2


@pytest.mark.parametrize('name', ['tiny_d16', 'd20_h24_depth3'])
def test_a_tagged_prefix_is_the_primed_decode(name, oracle_lib):
  case = golden_util.load_case(name)
  seq = case['seqs'][1][:14]
  prefix = [0, 0, 1, 0, 2]
  tags = np.zeros(len(seq), dtype=np.uint8)
  tags[:len(prefix)] = [7, 7, 3, 7, 100]
  got = known_ref.decode(case['params'], seq, 4, 1, 1, tags=tags)
  want = limit_ref.primed_decode(case['params'], seq, prefix, 4)
  assert np.array_equal(np.array([h.trace for h in got['beam']]), want['labels'])
  assert np.array_equal(_bits([h.score for h in got['beam']]), _bits(want['scores']))


def _consistent(labels, tags):
  """Equal tags, equal labels; different tags, different labels."""
  label_of = {}
  for lab, g in zip(labels, tags):
    if g and label_of.setdefault(int(g), int(lab)) != int(lab):
      return False
  return len(set(label_of.values())) == len(label_of)


@pytest.mark.parametrize('name', ['tiny_d16', 'toy_d2_depth2', 'd20_h24_depth3'])
@pytest.mark.parametrize('look_ahead,test_iteration', [(1, 1), (1, 2), (2, 1), (3, 2)])
def test_the_tags_hold_in_every_hypothesis(name, look_ahead, test_iteration, oracle_lib):
  case = golden_util.load_case(name)
  joined = 0
  for u, seq in enumerate(_short(case, 3, 12 if look_ahead < 3 else 8)):
    tags = known_ref.pattern(u, len(seq))
    got = known_ref.decode(case['params'], seq, 4 if look_ahead < 3 else 3, look_ahead, test_iteration, tags=tags)
    assert got['beam'], 'the pattern emptied the beam'
    n = len(seq)
    for hyp in got['beam']:
      assert _consistent(hyp.trace, np.tile(tags, test_iteration)), (u, hyp.trace)   # (bindings persist across passes)
      bound = {hyp.trace[t] for t in range(n) if tags[t]}
      joined += any(not tags[t] and hyp.trace[t] in bound for t in range(n))
  assert joined   # (a free frame may join a tagged cluster)


def test_the_contradictions_empty_the_beam(oracle_lib):
  case = golden_util.load_case('tiny_d16')
  seq = case['seqs'][0][:8]
  n = len(seq)
  two = np.array([0, 1, 0, 0, 2, 0, 0, 0], dtype=np.uint8)
  # two tags under max_speakers 1
  got = known_ref.decode(case['params'], seq, 4, 1, 1, limit=1, tags=two)
  assert not got['beam'] and got['labels'].tolist() == [-1] * n and np.isposinf(got['score'])
  assert known_ref.decode(case['params'], seq, 4, 1, 1, limit=2, tags=two)['beam']
  # a bias of 0 (stay) at a frame whose tag is bound to another cluster
  stay = np.full(n, np.nan)
  stay[4] = 0.0
  back = np.array([1, 0, 2, 2, 1, 0, 0, 0], dtype=np.uint8)
  assert not known_ref.decode(case['params'], seq, 4, 1, 1, bias=stay, tags=back)['beam']
  assert known_ref.decode(case['params'], seq, 4, 1, 1, tags=back)['beam']
  # every cluster bound and a new tag: only the new cluster is allowed -- and a limit that forbids it empties the beam
  third = np.array([1, 2, 1, 2, 3, 0, 0, 0], dtype=np.uint8)
  got = known_ref.decode(case['params'], seq, 4, 1, 1, tags=third)
  assert all(h.trace[:5] == [0, 1, 0, 1, 2] for h in got['beam']) and got['beam']
  assert not known_ref.decode(case['params'], seq, 4, 1, 1, limit=2, tags=third)['beam']
  # look_ahead 2: the same inside a window
  assert not known_ref.decode(case['params'], seq, 4, 2, 1, limit=2, tags=third)['beam']


# ---- the surface

def test_the_new_symbol_is_declared_bound_and_exported():
  header = open(os.path.join(_ROOT, 'include', 'uisrnn_hip.h')).read()
  assert re.search(r'int32_t uis_frame_speakers\(uis_handle\* h, const uint8_t\* tags, int64_t n_frames\);', header)
  assert 'uis_frame_speakers' in _capi.EXPORTED_SYMBOLS
  lib = _capi.load_library()
  assert lib.uis_frame_speakers.argtypes is not None
  assert lib.uis_frame_speakers(None, None, 0) == _capi.UIS_ERR_INVALID_ARG   # a null handle is refused, not dereferenced
  for fn in ('predict', 'predict_single', 'predict_nbest', 'predict_posteriors'):
    assert 'known_speakers' in getattr(uisrnn_amd.UISRNN, fn).__code__.co_varnames, fn
  assert 'known_speakers' in host.parallel_predict.__code__.co_varnames
  for fn in ('decode', 'decode_f64', 'decode_host', 'decode_device'):
    assert 'speakers' in getattr(_capi.Decoder, fn).__code__.co_varnames, fn


def test_the_keyword_as_the_librarys_table():
  check = host._check_known_speakers  # pylint: disable=protected-access
  assert check(None, [3, 2]) is None
  got = check([['bob', None, 'amy'], None], [3, 2])
  assert [g.tolist() for g in got] == [[1, 0, 2], [0, 0]] and all(g.dtype == np.uint8 for g in got)
  # names are numbered per utterance, by first appearance; any hashable value is a name (0 and '' too)
  got = check([[None, 'amy', 'bob', 'amy'], ['bob', 0, ('x', 1), '']], [4, 4])
  assert [g.tolist() for g in got] == [[0, 1, 2, 1], [1, 2, 3, 4]]
  assert check(['a', None, 'a'], [3], single=True)[0].tolist() == [1, 0, 1]
  assert check(np.array(['a', 'b', 'a']), [3], single=True)[0].tolist() == [1, 2, 1]
  assert check((), [0], single=True)[0].tolist() == []
  assert check([list(range(127)), None], [127, 1])[0].tolist() == list(range(1, 128))
  for bad in (True, np.bool_(False), 'ab', 5, [['a', 'b', 'c']], [['a', 'b'], ['a', 'b']], [['a', 'b', 'c'], ['a']],
              [['a', 'b', 'c'], True], [['a', 'b', 'c'], 'ab'], np.array([1, 2, 3, 4, 5])):
    with pytest.raises(ValueError):
      check(bad, [3, 2])
  for bad in (True, 'abc', ['a', 'b'], 7):
    with pytest.raises(ValueError):
      check(bad, [3], single=True)
  # names are dict keys: 1, 1.0 and True are one speaker; a NaN equals nothing and is refused
  assert check([[1, 1.0, True], [2, 1]], [3, 2])[0].tolist() == [1, 1, 1]
  for nan in (float('nan'), np.float32('nan'), np.array([0.5, np.nan, 0.5])[1]):
    with pytest.raises(ValueError, match='NaN'):
      check([['a', nan, 'a'], None], [3, 2])
  with pytest.raises(ValueError, match='NaN'):
    check(np.array([0.5, np.nan, 0.5]), [3], single=True)
  with pytest.raises(ValueError, match='more than 127'):
    check([list(range(128)), None], [128, 1])
  with pytest.raises(TypeError):
    check([['a', ['b'], 'c'], None], [3, 2])
  with pytest.raises(TypeError):
    check(['a', {}, 'c'], [3], single=True)


def test_invalid_values_raise_before_any_device_work():
  model = uisrnn_amd.UISRNN(types.SimpleNamespace(
      observation_dim=4, rnn_hidden_size=8, rnn_depth=1, rnn_dropout=0.0, transition_bias=None, crp_alpha=1.0,
      sigma2=None, verbosity=0, enable_cuda=False))

  def no_device(*unused_args, **unused_kwargs):
    raise AssertionError('reached the device')

  model._get_decoder = no_device   # pylint: disable=protected-access
  model._decode_batch = no_device  # pylint: disable=protected-access
  args = types.SimpleNamespace(beam_size=4, look_ahead=1, test_iteration=1)
  seqs = [np.zeros((3, 4)), np.zeros((2, 4))]
  calls = (lambda k: model.predict(seqs, args, known_speakers=k),
           lambda k: model.predict_nbest(seqs, args, known_speakers=k),
           lambda k: model.predict_posteriors(seqs, args, known_speakers=k),
           lambda k: host.parallel_predict(model, seqs, args, known_speakers=k))
  for bad in (True, [['a', 'b', 'c']], [['a', 'b'], ['a', 'b']], [['a', 'b', 'c'], True]):
    for call in calls:
      with pytest.raises(ValueError):
        call(bad)
  for call in calls:
    with pytest.raises(TypeError):
      call([['a', [], 'c'], None])
  many = [np.zeros((128, 4)), np.zeros((2, 4))]
  with pytest.raises(ValueError):
    model.predict(many, args, known_speakers=[list(range(128)), None])
  for bad in (True, ['a', 'b'], [['a', 'b', 'c'], ['a', 'b', 'c']]):
    with pytest.raises(ValueError):
      model.predict_single(seqs[0], args, known_speakers=bad)
    with pytest.raises(ValueError):
      model.predict(seqs[0], args, known_speakers=bad)
  with pytest.raises(TypeError):
    model.predict_single(seqs[0], args, known_speakers=['a', {}, 'c'])


# ---- the table follows the regroupings (stand-in decoders, as tests/test_front_end_host.py)

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


def _numbered(n_utt, need=()):
  """Utterance k: 3 + k % 4 frames, k in column 0, the level capacity it needs in column 1."""
  seqs = []
  for k in range(n_utt):
    s = np.zeros((3 + k % 4, DIM))
    s[:, 0] = k
    s[:, 1] = need[k] if k < len(need) else 100
    seqs.append(s)
  return seqs


def _names(seqs):
  """Utterance k names speaker k + 1 at every frame but its first: the table says whose it is."""
  return [[None] + ['s{}'.format(k)] * (s.shape[0] - 1) for k, s in enumerate(seqs)]


class _Regrouped:
  """decode_f64 that checks the speaker table it is handed against the numbers of the sequences it is handed; at most
  `room` utterances per call; utterance k needs a level capacity of its column 1, and overflows a cluster cap below
  `cap_need[k]`."""

  def __init__(self, room=99, cap_need=None):
    self.room, self.cap_need, self.calls, self.flags = room, cap_need or {}, [], np.zeros(0, dtype=np.int32)

  def decode_f64(self, seqs, beam_size, look_ahead, test_iteration, max_clusters=0, flags=0, level_cap=0, **tables):
    cap = level_cap or 32768
    numbers = [int(s[0, 0]) for s in seqs]
    self.calls.append((numbers, cap, max_clusters))
    assert sorted(tables) == ['speakers']
    table = tables['speakers']
    assert table.dtype == np.uint8 and table.shape == (sum(s.shape[0] for s in seqs),)
    at = 0
    for s in seqs:
      assert table[at:at + s.shape[0]].tolist() == [0] + [1] * (s.shape[0] - 1)
      at += s.shape[0]
    if len(seqs) > self.room:
      self.flags = np.zeros(0, dtype=np.int32)
      raise _error(_capi.UIS_ERR_OOM, 'decode state would need 999 GB')
    self.flags = np.array([2 if int(s[0, 1]) > cap else 0 for s in seqs], dtype=np.int32)
    if self.flags.any():
      raise _error(_capi.UIS_ERR_UNSUPPORTED, 'a look-ahead window held more prefixes than a level')
    labels = np.concatenate([np.full(s.shape[0], k, dtype=np.int32) for s, k in zip(seqs, numbers)])
    overflow = np.array([1 if max_clusters < self.cap_need.get(k, 0) else 0 for k in numbers], dtype=np.int32)
    return {'status': 0, 'labels': labels, 'overflow': overflow, 'stats': {'decode_kernel': 'stand-in'}}

  def last_overflow(self, n_utt=None):
    return self.flags


_NEED = [100, 40000, 100, 300000, 100, 100, 100, 100]


def test_the_table_follows_the_overflow_retry():
  model, args = _model()
  seqs = _numbered(7)
  dec = _Regrouped(cap_need={2: 40, 5: 100})
  model._get_decoder = lambda device=None: dec  # pylint: disable=protected-access
  out = model.predict(seqs, args, known_speakers=_names(seqs))
  assert out == [[k] * s.shape[0] for k, s in enumerate(seqs)]
  assert [numbers for numbers, _, _ in dec.calls][:2] == [list(range(7)), [2, 5]] and len(dec.calls) >= 3
  assert dec.calls[-1][0] == [5]


def test_the_table_follows_the_halves_after_oom_and_the_shards():
  model, args = _model()
  seqs = _numbered(11)
  dec = _Regrouped(room=3)
  model._get_decoder = lambda device=None: dec  # pylint: disable=protected-access
  out = model.predict(seqs, args, known_speakers=_names(seqs))
  assert out == [[k] * s.shape[0] for k, s in enumerate(seqs)]
  assert dec.calls[0][0] == list(range(11)) and dec.calls[1][0] == list(range(0, 11, 2))
  dec = _Regrouped(room=3)
  out = uisrnn_amd.parallel_predict(model, seqs, args, devices=[0], known_speakers=_names(seqs))
  assert out == [[k] * s.shape[0] for k, s in enumerate(seqs)]
  # a shard of a list is a _decode_batch of its members' tables (parallel_predict's workers call exactly this)
  shard = [7, 2, 9]
  speakers = host._check_known_speakers(_names(seqs), [s.shape[0] for s in seqs])  # pylint: disable=protected-access
  dec = _Regrouped()
  worker = types.SimpleNamespace(_model=model, _decoder=dec)
  out = host._Worker.decode(worker, [seqs[k] for k in shard], args, None, None, [speakers[k] for k in shard])  # pylint: disable=protected-access
  assert out == [[k] * seqs[k].shape[0] for k in shard] and dec.calls[0][0] == shard


@pytest.mark.parametrize('room', [99, 3])
def test_the_table_follows_the_look_ahead_retry_groups(room):
  model, args = _model(look_ahead=3)
  seqs = _numbered(8, _NEED)
  dec = _Regrouped(room=room)
  model._get_decoder = lambda device=None: dec  # pylint: disable=protected-access
  out = model.predict(seqs, args, known_speakers=_names(seqs))
  assert out == [[k] * s.shape[0] for k, s in enumerate(seqs)]
  assert sorted({cap for _, cap, _ in dec.calls}) == [32768, 262144, 524287]
  # (utterance 3 needs the largest capacity: it got there, with its rows of the table -- _Regrouped checked them)
  assert any(3 in numbers and cap == 524287 for numbers, cap, _ in dec.calls)
  assert room < 99 or [1, 3] in [numbers for numbers, _, _ in dec.calls]


def test_without_known_speakers_the_decoder_receives_no_keyword():
  model, args = _model()
  seqs = _numbered(3)
  seen = []

  class _Plain:
    def decode_f64(self, seqs, beam_size, look_ahead, test_iteration, max_clusters=0, flags=0, level_cap=0, **tables):
      seen.append(sorted(tables))
      return {'status': 0, 'labels': np.zeros(sum(s.shape[0] for s in seqs), dtype=np.int32),
              'overflow': np.zeros(len(seqs), dtype=np.int32), 'stats': {}}

  model._get_decoder = lambda device=None: _Plain()  # pylint: disable=protected-access
  model.predict(seqs, args)
  model.predict(seqs, args, known_speakers=None)
  assert seen == [[], []]
