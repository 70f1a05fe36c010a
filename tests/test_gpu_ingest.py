"""k_ingest (csrc/uis_ingest.hip) through uis_ingest_tensors, against tests/ingest_ref.py, bit for bit (NaN as NaN).

The packed float32 stream the gather leaves must be what numpy makes of the tensors' VALUES: float64 rounded to nearest
even with subnormal results and overflow (the rounding of uis_decode_f64's cast and of astype(float32)), float16 and
bfloat16 exact -- this test decides whether gfx950's converts honour that under the library's denormal mode -- for
every addressing the descriptor allows: every dtype x D in {1, 3, 4, 8, 255, 256}, 0 / 1 / 2 rows and one row more than
a workgroup takes, slices of a padded batch, a [:, :D] view, a base off 16-byte alignment, a row pitch under which
alignment alternates row by row, an output base off 16-byte alignment.  Every output buffer is pre-filled and two rows
longer than the stream: what lies behind the stream must stay as it was.
"""

import ctypes

import numpy as np
import pytest
import torch

import ingest_ref as ref
from uisrnn_amd import _capi
from uisrnn_amd import weights

pytestmark = pytest.mark.gpu

DIMS = (1, 3, 4, 8, 255, 256)
DTYPES = (torch.float64, torch.float32, torch.float16, torch.bfloat16)
FILL = 0x7fc12345   # a NaN no conversion produces
KNOB = 'UIS_POISON_WORKSPACE'


@pytest.fixture(scope='module')
def decoders():
  made = {}

  def get(dim):
    if dim not in made:
      made[dim] = _capi.Decoder(weights.init_params(dim, 16, 1, sigma2=0.1, transition_bias=0.05, crp_alpha=1.0, seed=dim))
    return made[dim]
  yield get
  for dec in made.values():
    dec.close()


def _values(shape, dtype, seed):
  g = torch.Generator().manual_seed(seed)
  return (torch.randn(shape, generator=g, dtype=torch.float64) * 3).to(dtype).cuda()


def _same(got, want, what):
  got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  nan = np.isnan(want)
  assert np.array_equal(np.isnan(got), nan), what
  bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
  assert not bad.any(), (what, int(bad.sum()), got[bad][:4], want[bad][:4])


def _ingest(dec, tensors, dim, what, lengths=None, offset_floats=0):
  """One uis_ingest_tensors into a pre-filled buffer whose base is offset_floats floats behind a 16-byte boundary."""
  listed = tensors if lengths is None else [tensors[u, :n] for u, n in enumerate(lengths)]
  want = ref.expected(listed, dim)
  rows = want.shape[0]
  buf = torch.full(((rows + 2) * dim + offset_floats,), FILL, dtype=torch.int32, device='cuda').view(torch.float32)
  out = buf[offset_floats:].view(rows + 2, dim)
  assert out.data_ptr() % 16 == (4 * offset_floats) % 16
  got = dec.ingest_tensors(tensors, lengths=lengths, out=out)
  assert got.shape == (rows, dim) and (rows == 0 or got.data_ptr() == out.data_ptr()), what
  _same(got.cpu().numpy(), want, what)
  assert (buf.view(torch.int32).cpu().numpy()[offset_floats + rows * dim:] == FILL).all(), (what, 'wrote past the stream')
  assert (buf.view(torch.int32).cpu().numpy()[:offset_floats] == FILL).all(), (what, 'wrote before the stream')


def _name(dtype):
  return str(dtype).split('.')[1]


@pytest.mark.parametrize('dim', DIMS)
@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
def test_every_dtype_and_width_at_the_row_counts_where_the_grid_changes(dtype, dim, decoders):
  dec = decoders(dim)
  more = _capi.ingest_workgroup_rows(dim) + 1   # one row more than a workgroup takes: a second workgroup, nearly idle
  for rows in (0, 1, 2, more):
    _ingest(dec, [_values((rows, dim), dtype, rows)], dim, (_name(dtype), dim, rows))
  # ... and as the blocks of one call, an absent one among them: rows of several blocks inside one workgroup
  blocks = [_values((2, dim), dtype, 11), _values((0, dim), dtype, 12), None, _values((1, dim), dtype, 13),
            _values((more, dim), dtype, 14), _values((0, dim), dtype, 15)]
  _ingest(dec, blocks, dim, (_name(dtype), dim, 'blocks'))
  _ingest(dec, blocks, dim, (_name(dtype), dim, 'blocks, output base 8 bytes off'), offset_floats=2)


def test_blocks_of_different_dtypes_in_one_call(decoders):
  blocks = [_values((5, 8), dt, 20 + k) for k, dt in enumerate(DTYPES)] + [_values((70, 8), torch.float16, 30)]
  _ingest(decoders(8), blocks, 8, 'mixed dtypes')


@pytest.mark.parametrize('dim', [3, 8, 256])
@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
def test_slices_of_a_padded_batch_and_a_view_of_a_wider_tensor(dtype, dim, decoders):
  dec = decoders(dim)
  batch = _values((5, 9, dim), dtype, 40)
  lengths = [9, 4, 0, 1, 7]
  _ingest(dec, [batch[u, :n] for u, n in enumerate(lengths)], dim, (_name(dtype), dim, 'slices'))
  _ingest(dec, batch, dim, (_name(dtype), dim, 'batch + lengths'), lengths=lengths)
  wide = _values((37, 2 * dim), dtype, 41)
  _ingest(dec, [wide[:, :dim]], dim, (_name(dtype), dim, '[:, :D]'))
  _ingest(dec, [wide[:, dim:]], dim, (_name(dtype), dim, '[:, D:]'))
  cut = _values((3, 6, 2 * dim), dtype, 42)[:, :, :dim]    # a batch whose rows are the left halves of wider ones
  _ingest(dec, cut, dim, (_name(dtype), dim, 'batch of views'), lengths=[6, 2, 5])


def test_a_base_off_16_byte_alignment(decoders):
  """f16, D = 3, from the second row: the base is 6 bytes behind a 16-byte boundary."""
  t = _values((40, 3), torch.float16, 50)
  assert t.data_ptr() % 16 == 0 and t[1:].data_ptr() % 16 == 6
  _ingest(decoders(3), [t[1:]], 3, 'f16 D 3 t[1:]')
  # the same at a width the vector path would take if the base allowed it
  t8 = _values((40, 8), torch.bfloat16, 51).view(-1)[4:4 + 39 * 8].view(39, 8)
  assert t8.data_ptr() % 16 == 8
  _ingest(decoders(8), [t8], 8, 'bf16 D 8, base 8 bytes off')


def test_a_row_pitch_under_which_alignment_alternates(decoders):
  """f16, D = 4, row stride 6 elements = 12 bytes: the base and every fourth row are 16-byte aligned, the others are
  not -- the block must go the scalar way (or align per row)."""
  base = _values((6 * 50,), torch.float16, 60)
  t = torch.as_strided(base, (50, 4), (6, 1))
  assert t.data_ptr() % 16 == 0 and (t.stride(0) * 2) % 16 == 12
  _ingest(decoders(4), [t], 4, 'f16 D 4 stride 6')
  f32 = torch.as_strided(_values((6 * 50,), torch.float32, 61), (50, 4), (6, 1))   # 24 bytes: every other row
  _ingest(decoders(4), [f32], 4, 'f32 D 4 stride 6')
  f64 = torch.as_strided(_values((5 * 50,), torch.float64, 62), (50, 4), (5, 1))   # 40 bytes
  _ingest(decoders(4), [f64], 4, 'f64 D 4 stride 5')


def _hostile_f64():
  f = np.float64
  flt_max, tiny, sub = f(np.finfo(np.float32).max), f(2.0) ** -126, f(2.0) ** -149
  values = [
      0.0, np.inf, np.nan, 1.0, flt_max, np.nextafter(flt_max, np.inf),   # the largest normal, and just over it
      flt_max + f(2.0) ** 103,                        # half an ulp over: a tie, to even = 2^128 = inf
      np.nextafter(flt_max + f(2.0) ** 103, 0.0),     # just under the tie: FLT_MAX
      f(2.0) ** 128, 1e300,
      tiny, np.nextafter(tiny, 0.0),                  # the smallest normal; just under it: rounds up to it
      tiny - f(2.0) ** -150,                          # tie between the largest subnormal (odd) and 2^-126 (even)
      tiny - sub, tiny - sub - f(2.0) ** -151,        # the largest subnormal, and a value that rounds to it
      sub, 1.5 * sub,                                 # the smallest subnormal; a tie between 1 (odd) and 2 (even) units
      2.5 * sub,                                      # a tie between 2 (even) and 3: down
      0.5 * sub,                                      # a tie between 0 (even) and the smallest subnormal: 0
      np.nextafter(0.5 * sub, 1.0),                   # just over it: the smallest subnormal
      0.25 * sub, 5e-324,                             # below half the smallest subnormal; float64's own smallest
      1.0 + f(2.0) ** -24, 1.0 + 3 * f(2.0) ** -24,   # ties in the normal range: to even, down and up
      np.nextafter(1.0 + f(2.0) ** -24, 2.0), 1.0 / 3.0,
  ]
  values = np.array(values + [-v for v in values], dtype=np.float64)
  want = ref.convert(values, ref.F64)
  # (the reference is what the test says it is)
  assert np.isinf(want[6]) and want[7] == np.finfo(np.float32).max and want[11] == np.float32(2.0) ** -126
  assert want[12] == np.float32(2.0) ** -126 and want[16].view(np.uint32) == 2 and want[18] == 0 and want[19].view(np.uint32) == 1
  return values


@pytest.mark.parametrize('dim', [4, 3])
def test_float64_rounds_as_the_host_cast_at_the_edges_of_float32(dim, decoders):
  """Largest and smallest normals and subnormals, ties to even at both, just over FLT_MAX, +-0, +-inf, NaN -- through
  the 16-byte path (D 4) and the scalar one (D 3)."""
  values = _hostile_f64()
  values = np.concatenate([values, np.ones(-len(values) % (4 * 3))])
  t = torch.from_numpy(values.reshape(-1, dim)).cuda()
  _ingest(decoders(dim), [t], dim, ('hostile f64', dim))


@pytest.mark.parametrize('dim', [8, 4, 3])
@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16], ids=_name)
def test_every_16_bit_pattern_converts_exactly(dtype, dim, decoders):
  """All 65536 bit patterns of float16 and of bfloat16 -- subnormals, infinities and NaNs among them -- through the
  8-element path (D 8), the 4-element path (D 4) and the scalar path (D 3)."""
  n = 65536 // dim * dim
  bits = torch.arange(n, dtype=torch.int32).to(torch.int16).view(dtype).view(-1, dim).cuda()
  _ingest(decoders(dim), [bits], dim, (_name(dtype), dim, 'every pattern'))


@pytest.mark.parametrize('word', ['ffffffff', '7f7f7f7f'])
def test_under_workspace_poison(word, monkeypatch, decoders):
  monkeypatch.setenv(KNOB, word)
  for dim in (3, 8):
    blocks = [_values((2, dim), torch.float64, 70), None, _values((_capi.ingest_workgroup_rows(dim) + 1, dim), torch.float16, 71),
              _values((5, 2 * dim), torch.bfloat16, 72)[:, :dim]]
    _ingest(decoders(dim), blocks, dim, ('poison', word, dim))


def test_the_library_refuses_bad_lists_before_any_gpu_work(decoders):
  dec = decoders(4)
  good = _values((3, 4), torch.float32, 80)
  out = torch.zeros(8, 4, device='cuda')
  lib, handle = dec._lib, dec._handle   # pylint: disable=protected-access

  def call(records, capacity=8, out_ptr=out.data_ptr()):
    table = np.zeros(len(records), dtype=_capi.TENSOR_RECORD)
    for i, rec in enumerate(records):
      table[i] = rec
    return lib.uis_ingest_tensors(handle, ctypes.c_void_p(table.ctypes.data), len(table), None, ctypes.c_void_p(out_ptr), capacity)

  ok = (good.data_ptr(), 3, 4, _capi.UIS_DTYPE_F32, 0)
  assert call([ok]) == _capi.UIS_OK and torch.equal(out[:3], good)
  for name, records, kw in (('null data with rows', [(0, 3, 4, 0, 0)], {}), ('negative rows', [(good.data_ptr(), -1, 4, 0, 0)], {}),
                            ('unknown dtype', [(good.data_ptr(), 3, 4, 4, 0)], {}), ('row_stride below D', [(good.data_ptr(), 3, 3, 0, 0)], {}),
                            ('misaligned', [(good.data_ptr() + 4, 1, 4, _capi.UIS_DTYPE_F64, 0)], {}),
                            ('capacity_rows too small', [ok, ok, ok], {}), ('no output', [ok], {'out_ptr': None}),
                            ('the second block', [ok, (0, 1, 4, 0, 0)], {})):
    assert call(records, **kw) == _capi.UIS_ERR_INVALID_ARG, name
    assert _capi.last_error(lib), name
  assert lib.uis_ingest_tensors(handle, None, -1, None, None, 0) == _capi.UIS_ERR_INVALID_ARG
  assert lib.uis_ingest_tensors(handle, None, 0, None, None, 0) == _capi.UIS_OK       # nothing to do
  assert call([(0, 0, 0, 0, 0), ok, (0, 0, 4, 2, 0)]) == _capi.UIS_OK                 # rows 0: no data, any stride
  # the wrapper says the same in Python's words, before the library
  with pytest.raises(ValueError):
    dec.ingest_tensors([good, good, good], out=out[:8].view(8, 4)[:5])   # (5 rows of room for 9)
  with pytest.raises(TypeError):
    dec.ingest_tensors([good.cpu()])
  with pytest.raises(TypeError):
    dec.ingest_tensors([good.to(torch.int32)])
  with pytest.raises(ValueError):
    dec.ingest_tensors([_values((3, 5), torch.float32, 81)])
