"""Device tensors in, the host side (no GPU): the uis_tensor table the front end builds from torch tensors and views,
the checks that hold before the library is called, and predict_tensors' path through _decode_batch with a stand-in
decoder, as tests/test_front_end_host.py does it for predict.

The tables are built from CPU tensors here (device=None skips the device check): a descriptor is addresses, strides
and a dtype code, whatever memory the address points into.  tests/ingest_ref.py states what a table means.
"""

import inspect
import os
import re

import numpy as np
import pytest
import torch

import ingest_ref as ref
import uisrnn_amd
from uisrnn_amd import _capi
from uisrnn_amd import arguments

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
DTYPES = {torch.float32: ref.F32, torch.float64: ref.F64, torch.float16: ref.F16, torch.bfloat16: ref.BF16}


def _base(n, dtype, seed=0):
  """A flat tensor of n distinct values that every dtype here holds exactly (multiples of 1/8 below 256)."""
  g = torch.Generator().manual_seed(seed)
  return (torch.randint(-2040, 2040, (n,), generator=g).to(torch.float64) / 8).to(dtype)


def _storage(base):
  return base.view(torch.int16).numpy().view(np.uint16) if base.dtype == torch.bfloat16 else base.numpy()


def _blocks(table, base):
  """The table as ingest_ref's blocks over `base`'s storage (every tensor described is a view of `base`)."""
  esz = base.element_size()
  out = []
  for rec in table:
    start = (int(rec['data']) - base.data_ptr()) // esz if rec['rows'] else 0
    assert not rec['rows'] or (int(rec['data']) - base.data_ptr()) % esz == 0
    out.append({'storage': _storage(base), 'start': start, 'rows': int(rec['rows']), 'row_stride': int(rec['row_stride']),
                'dtype': int(rec['dtype']), 'data': int(rec['data'])})
  return out


def _views(base, dim):
  """Views of one flat tensor: (name, list for tensor_table)."""
  n = base.numel()
  batch = base[:4 * 6 * dim].view(4, 6, dim)
  wide = base[:5 * 2 * dim].view(5, 2 * dim)
  return [
      ('contiguous', [base[:7 * dim].view(7, dim)]),
      ('slices of a batch', [batch[0, :6], batch[1, :2], batch[2, :0], batch[3, :5]]),
      ('left half of a wide tensor', [wide[:, :dim]]),
      ('right half: base off the row start', [wide[:, dim:]]),
      ('from the second row', [base[:7 * dim].view(7, dim)[1:]]),
      ('an absent slot between two', [base[:dim].view(1, dim), None, base[dim:3 * dim].view(2, dim)]),
      ('one row of a wide tensor', [wide[2:3, :dim]]),
      ('padded rows', [torch.as_strided(base, (3, dim), (dim + 2, 1))]),
      ('nothing', []),
  ] if n >= 4 * 6 * dim else []


@pytest.mark.parametrize('dtype', list(DTYPES), ids=[str(d).split('.')[1] for d in DTYPES])
@pytest.mark.parametrize('dim', [1, 3, 4, 8])
def test_the_table_of_views_is_their_addresses_strides_and_dtype(dtype, dim):
  base = _base(400, dtype)
  for name, tensors in _views(base, dim):
    table, keep = _capi.tensor_table(tensors, dim)
    assert table.dtype == _capi.TENSOR_RECORD and table.dtype.itemsize == 32 and len(table) == len(tensors), name
    assert len(keep) == sum(t is not None for t in tensors), name
    for rec, t in zip(table, tensors):
      if t is None or t.shape[0] == 0:
        assert rec['rows'] == 0, name
        continue
      assert int(rec['data']) == t.data_ptr() and int(rec['rows']) == t.shape[0] and int(rec['dtype']) == DTYPES[dtype], name
      assert int(rec['row_stride']) == (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), dim)), name
      assert int(rec['reserved']) == 0
    blocks = _blocks(table, base)
    assert ref.refusal(blocks, dim) is None and _capi.check_tensor_table(table, dim) == sum(b['rows'] for b in blocks), name
    got, want = ref.gather(blocks, dim), ref.expected(tensors, dim)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    for out_address in (0, 4096, 4104):
      flags = _capi.tensor_vector_flags(table, dim, out_address)
      want_flags = [ref.vector_flag(b['data'], b['rows'], b['row_stride'], b['dtype'], dim, out_address) for b in blocks]
      assert flags.tolist() == want_flags, (name, out_address)


def test_the_batch_form_is_the_list_of_its_slices():
  base = _base(4 * 6 * 8, torch.float16)
  batch = base.view(4, 6, 8)
  lengths = [6, 2, 0, 5]
  table, _ = _capi.tensor_table(batch, 8, lengths)
  listed, _ = _capi.tensor_table([batch[u, :n] for u, n in enumerate(lengths)], 8)
  for a, b in zip(table, listed):
    assert int(a['rows']) == int(b['rows']) and int(a['dtype']) == int(b['dtype'])
    if a['rows'] > 1:
      assert int(a['data']) == int(b['data']) and int(a['row_stride']) == int(b['row_stride'])
  whole, _ = _capi.tensor_table(batch, 8)
  assert whole['rows'].tolist() == [6] * 4
  # a batch cut out of a wider one: utterances 48 + 16 elements apart, rows 8 + 8
  wide = _base(3 * 4 * 16, torch.float32).view(3, 4, 16)
  table, _ = _capi.tensor_table(wide[:, :, :8], 8, torch.tensor([4, 1, 3]))
  assert table['row_stride'].tolist() == [16] * 3 and table['rows'].tolist() == [4, 1, 3]
  assert [int(p) - wide.data_ptr() for p in table['data']] == [0, 4 * 16 * 4, 2 * 4 * 16 * 4]
  for bad in ([6, 2, 0], [6, 2, 0, 7], [6, 2, -1, 5]):
    with pytest.raises(ValueError):
      _capi.tensor_table(batch, 8, bad)
  with pytest.raises(ValueError):
    _capi.tensor_table([batch[0]], 8, [6])   # (lengths belongs to the batch form)


def test_the_alignment_cases_named_by_the_kernel():
  """f16, D = 3 from the second row: a base 6 bytes off.  f16, D = 4, row stride 6: the base is aligned, every other
  row is not -- no 16-byte access.  The same tensor with stride 8: vector."""
  base = _base(64, torch.float16)
  assert base.data_ptr() % 16 == 0
  off = base[:30].view(10, 3)[1:]
  alternating = torch.as_strided(base, (5, 4), (6, 1))
  aligned = torch.as_strided(base, (5, 4), (8, 1))
  for t, dim, want in ((off, 3, False), (alternating, 4, False), (aligned, 4, True)):
    table, _ = _capi.tensor_table([t], dim)
    assert _capi.tensor_vector_flags(table, dim).tolist() == [want]
    assert ref.vector_flag(t.data_ptr(), t.shape[0], t.stride(0), ref.F16, dim) == want
  # an aligned block whose place in the stream is not (the output base 8 bytes off): no vector access either
  table, _ = _capi.tensor_table([aligned], 4)
  assert _capi.tensor_vector_flags(table, 4, 4104).tolist() == [False]


def test_a_non_unit_inner_stride_or_overlapping_rows_are_made_contiguous():
  base = _base(48, torch.float32)
  transposed = base.view(4, 12).t()[:, :4]           # [12, 4] with inner stride 12
  expanded = base[:4].view(1, 4).expand(5, 4)        # row stride 0
  for t in (transposed, expanded):
    table, keep = _capi.tensor_table([t], 4)
    assert keep[0].is_contiguous() and keep[0].data_ptr() != t.data_ptr() and torch.equal(keep[0], t)
    assert int(table[0]['data']) == keep[0].data_ptr() and int(table[0]['row_stride']) == 4
  column = base[:12].view(4, 3)[:, 1:2]              # D = 1: the inner stride of a size-1 dimension is nobody's business
  table, keep = _capi.tensor_table([column], 1)
  assert keep[0].data_ptr() == column.data_ptr() and int(table[0]['row_stride']) == 3


def _table(*records):
  table = np.zeros(len(records), dtype=_capi.TENSOR_RECORD)
  for i, rec in enumerate(records):
    table[i] = rec
  return table


@pytest.mark.parametrize('name,records,capacity', [
    ('null data with rows', [(0, 3, 4, 0, 0)], None),
    ('negative rows', [(4096, -1, 4, 0, 0)], None),
    ('unknown dtype', [(4096, 3, 4, 4, 0)], None),
    ('unknown dtype, negative', [(4096, 3, 4, -1, 0)], None),
    ('row_stride below D', [(4096, 3, 3, 0, 0)], None),
    ('misaligned float64', [(4100, 3, 4, 1, 0)], None),
    ('capacity_rows too small', [(4096, 3, 4, 0, 0), (8192, 2, 4, 2, 0)], 4),
    ('the second block', [(4096, 3, 4, 0, 0), (0, 1, 4, 0, 0)], None),
])
def test_every_validation_error_is_raised_before_the_library(name, records, capacity):
  table = _table(*records)
  blocks = [{'data': int(r['data']), 'rows': int(r['rows']), 'row_stride': int(r['row_stride']), 'dtype': int(r['dtype'])}
            for r in table]
  assert ref.refusal(blocks, 4, capacity) is not None, name
  with pytest.raises(ValueError):
    _capi.check_tensor_table(table, 4, capacity)


def test_what_the_library_accepts_passes():
  table = _table((0, 0, 0, 0, 0), (4096, 1, 4, 3, 0), (8192, 5, 9, 1, 0), (4098, 2, 4, 2, 0))
  assert _capi.check_tensor_table(table, 4, 8) == 8
  assert _capi.check_tensor_table(_table(), 4, 0) == 0


def test_front_end_type_errors_come_before_the_library():
  good = torch.zeros(3, 4)
  for bad, error in ((np.zeros((3, 4)), TypeError), ([[0.0] * 4], TypeError), (torch.zeros(3, 4, dtype=torch.int32), TypeError),
                     (torch.zeros(3, 4, dtype=torch.bool), TypeError), (torch.zeros(3, 4, dtype=torch.complex64), TypeError),
                     (torch.zeros(3, 5), ValueError), (torch.zeros(4), ValueError), (torch.zeros(2, 3, 4), ValueError)):
    with pytest.raises(error):
      _capi.tensor_table([good, bad], 4)
  # a tensor that is not on a GPU, asked for by a model on cuda:0 (no device needed to say so)
  with pytest.raises(TypeError, match='cpu'):
    _capi.tensor_table([good], 4, device=0)
  with pytest.raises(TypeError, match='meta'):
    _capi.tensor_table([torch.zeros(3, 4, device='meta')], 4, device=0)


def _model(**inference):
  model_args, _, inference_args = arguments.parse_arguments([])
  model_args.observation_dim = 4
  for key, value in inference.items():
    setattr(inference_args, key, value)
  return uisrnn_amd.UISRNN(model_args), inference_args


def test_predict_tensors_refuses_bad_arguments_before_any_decoder_exists():
  model, args = _model()
  model._get_decoder = lambda device=None: pytest.fail('the library was reached')  # pylint: disable=protected-access
  for bad, error in ((torch.zeros(3, 4), TypeError),                          # on the CPU
                     ([torch.zeros(3, 4)], TypeError),
                     (np.zeros((3, 4)), TypeError),                           # predict's argument
                     (torch.zeros(3, 4, dtype=torch.int64), TypeError),
                     ((torch.zeros(3, 4),), TypeError)):                      # neither a list nor a tensor
    with pytest.raises(error):
      model.predict_tensors(bad, args)
  model.device_index = None   # (any device: the remaining checks, on CPU tensors)
  for bad, kw, error in ((torch.zeros(3, 5), {}, ValueError), (torch.zeros(3, 4), {'lengths': [3]}, ValueError),
                         (torch.zeros(2, 3, 4), {'lengths': [3, 4]}, ValueError),
                         ([torch.zeros(3, 4)], {'max_speakers': [1, 2]}, ValueError),
                         ([torch.zeros(3, 4)], {'transition_bias': [np.zeros(2)]}, ValueError),
                         ([torch.zeros(3, 4)], {'min_turn': -1}, ValueError)):
    with pytest.raises(error):
      model.predict_tensors(bad, args, **kw)
  assert model.predict_tensors([], args) == []


def _error(status, text):
  err = _capi.HipLibraryError('stand-in failed ({}): {}'.format(status, text))
  err.status = status
  return err


class _StandIn:
  """decode_f64 and decode_tensors over the same rules: at most `room` utterances per call (else UIS_ERR_OOM);
  utterance k (its tag: column 0) overflows the cluster cap below NEED[k]; every table it is handed must be the
  tagged utterances' own."""
  NEED = {2: 64, 5: 32}

  def __init__(self, room):
    self.room, self.calls = room, []

  def _decode(self, seqs, max_clusters, tables, device):
    tags = [int(s[0, 0]) for s in seqs]
    self.calls.append((tags, max_clusters))
    assert sorted(tables) == ['bias', 'limits', 'min_turn', 'speakers'], sorted(tables)
    assert list(tables['limits']) == [t + 1 for t in tags] and list(tables['min_turn']) == [t + 2 for t in tags]
    at = 0
    for s, t in zip(seqs, tags):
      n = s.shape[0]
      assert (tables['bias'][at:at + n] == (t + 1) / 16).all() and (tables['speakers'][at:at + n] == 1 + t % 3).all(), t
      at += n
    if len(seqs) > self.room:
      raise _error(_capi.UIS_ERR_OOM, 'decode state would need 999 GB')
    overflow = np.array([int(max_clusters < self.NEED.get(t, 0)) for t in tags], dtype=np.int32)
    labels = np.concatenate([np.full(s.shape[0], t, dtype=np.int32) for s, t in zip(seqs, tags)])
    out = {'status': 0, 'overflow': overflow, 'stats': {}, 'scores': np.array(tags, dtype=np.float32) / 4}
    if device:
      out.update(labels=torch.from_numpy(labels), empty=np.zeros(len(seqs), dtype=bool))
    else:
      out.update(labels=labels)
    return out

  def decode_f64(self, seqs, beam_size, look_ahead, test_iteration, max_clusters=0, flags=0, level_cap=0, **tables):
    assert all(isinstance(s, np.ndarray) for s in seqs)
    return self._decode(seqs, max_clusters, tables, False)

  def decode_tensors(self, seqs, beam_size, look_ahead, test_iteration, max_clusters=0, flags=0, level_cap=0, **tables):
    assert all(isinstance(s, torch.Tensor) for s in seqs)
    return self._decode(seqs, max_clusters, tables, True)


def _tagged(n_utt):
  seqs = []
  for k in range(n_utt):
    s = np.zeros((3 + k % 4, 4))
    s[:, 0] = k
    seqs.append(s)
  return seqs


@pytest.mark.parametrize('room', [99, 3])
def test_predict_tensors_regroups_as_predict_and_each_utterance_keeps_its_tables(room):
  seqs = _tagged(9)
  rules = dict(max_speakers=[k + 1 for k in range(9)], transition_bias=[np.full(len(s), (k + 1) / 16) for k, s in enumerate(seqs)],
               known_speakers=[['abc'[k % 3]] * len(s) for k, s in enumerate(seqs)], min_turn=[k + 2 for k in range(9)])
  # (names are numbered 1 .. per utterance by first appearance: one name each, tag 1 -- the stand-in wants 1 + k % 3)
  model, args = _model()
  host, dev = _StandIn(room), _StandIn(room)

  def tags_of(k):
    return np.full(len(seqs[k]), 1 + k % 3, dtype=np.uint8)

  limits, bias, turns = rules['max_speakers'], rules['transition_bias'], rules['min_turn']
  speakers = [tags_of(k) for k in range(9)]
  want = model._decode_batch(seqs, args, decoder=host, limits=limits, bias=bias, speakers=speakers, min_turn=turns)  # pylint: disable=protected-access
  scores = [None] * 9
  got = model._decode_batch([torch.from_numpy(s) for s in seqs], args, decoder=dev, limits=limits, bias=bias,  # pylint: disable=protected-access
                            speakers=speakers, min_turn=turns, tensors=True, scores_out=scores)
  assert dev.calls == host.calls and len(host.calls) > (3 if room == 3 else 2)
  assert any(cap >= 64 for _, cap in dev.calls)   # (the overflowing utterances went back with more room)
  assert all(isinstance(g, torch.Tensor) and g.dtype == torch.int32 for g in got)
  assert [g.tolist() for g in got] == want == [[k] * len(s) for k, s in enumerate(seqs)]
  assert scores == [np.float32(k) / 4 for k in range(9)]


def test_predict_tensors_hands_the_checked_tables_to_the_same_path():
  """The list form and the [U, T, D] + lengths form, with all four rule tables, through predict_tensors itself."""
  tags, sizes = [0, 3, 6], [5, 2, 4]   # (one name per utterance is tag 1 = 1 + tag % 3)
  rules = dict(max_speakers=[t + 1 for t in tags], transition_bias=[np.full(n, (t + 1) / 16) for t, n in zip(tags, sizes)],
               known_speakers=[['anna'] * n for n in sizes], min_turn=[t + 2 for t in tags])
  model, args = _model()
  model.device_index = None   # (any device: the stand-in reads CPU tensors)
  batch = torch.zeros(3, 5, 4, dtype=torch.float16)
  for k, t in enumerate(tags):
    batch[k, :, 0] = t
  for source, more in (([batch[k, :n] for k, n in enumerate(sizes)], {}), (batch, {'lengths': sizes})):
    dev = _StandIn(99)
    model._get_decoder = lambda device=None, dev=dev: dev  # pylint: disable=protected-access
    labels, scores = model.predict_tensors(source, args, return_scores=True, **more, **rules)
    assert [lab.tolist() for lab in labels] == [[t] * n for t, n in zip(tags, sizes)]
    assert scores.dtype == np.float32 and scores.tolist() == [t / 4 for t in tags]
    assert dev.calls == [(tags, 16)]
  # a single [N, D] tensor: its one result, its one score
  dev = _StandIn(99)
  model._get_decoder = lambda device=None: dev  # pylint: disable=protected-access
  labels, score = model.predict_tensors(batch[1, :2], args, max_speakers=4, transition_bias=np.full(2, 4 / 16),
                                        known_speakers=['anna', 'anna'], min_turn=5, return_scores=True)
  assert labels.tolist() == [3, 3] and score == np.float32(0.75)


def test_the_symbols_are_declared_bound_and_named_outside_the_enumerated_prefixes():
  names = ('uis_ingest_tensors', 'uis_tensors_decode', 'uis_tensors_stream_push')
  assert set(names) <= set(_capi.EXPORTED_SYMBOLS) and _capi.UIS_ABI_VERSION == 6
  with open(os.path.join(ROOT, 'include', 'uisrnn_hip.h')) as f:
    header = f.read()
  for name in names:
    assert re.search(r'^int32_t %s\(uis_handle\* h, const uis_tensor\* ' % name, header, re.M), name
    assert not name.startswith(('uis_decode', 'uis_stream_', 'uis_score_'))   # (tests/test_gpu_call_tables.py enumerates those)
  assert re.search(r'typedef struct uis_tensor \{\s*const void\* data;[^}]*int64_t rows;[^}]*int64_t row_stride;[^}]*int32_t dtype;'
                   r'[^}]*int32_t reserved;[^}]*\} uis_tensor;', header)
  lib = _capi.load_library()
  assert lib.uis_ingest_tensors(None, None, 0, None, None, 0) == _capi.UIS_ERR_INVALID_ARG   # a null handle is refused
  assert lib.uis_tensors_decode(None, None, 0, None, None, None, None, None) == _capi.UIS_ERR_INVALID_ARG
  assert lib.uis_tensors_stream_push(None, None, None) == _capi.UIS_ERR_INVALID_ARG
  for cls, method in ((uisrnn_amd.UISRNN, 'predict_tensors'), (uisrnn_amd.OnlineSession, 'push_tensors'),
                      (uisrnn_amd.StreamPool, 'push_tensors'), (_capi.Decoder, 'decode_tensors'),
                      (_capi.Decoder, 'stream_push_tensors'), (_capi.Decoder, 'ingest_tensors')):
    assert callable(getattr(cls, method)), (cls, method)
  assert list(inspect.signature(uisrnn_amd.UISRNN.predict_tensors).parameters)[1:] == [
      'test_sequences', 'args', 'lengths', 'max_speakers', 'transition_bias', 'known_speakers', 'min_turn', 'return_scores']
  assert _capi.ingest_workgroup_rows(256) == 16 and _capi.ingest_workgroup_rows(3) == 512
