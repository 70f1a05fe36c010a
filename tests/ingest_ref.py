"""What a uis_tensor list means (include/uisrnn_hip.h, "Device tensors in"), stated in numpy: the reference of
tests/test_tensors_host.py, tests/test_gpu_ingest.py and tests/test_gpu_tensors.py.

A block is {storage, start, rows, row_stride, dtype}: row r, column c of the block is element start + r * row_stride + c
of the flat `storage`, and the packed stream is the blocks' rows in list order, converted to float32:
  float64   numpy's astype(float32): round to nearest even, subnormal results kept, overflow to +-inf
  float32   as it is
  float16   exact (numpy's astype)
  bfloat16  the 16 bits (storage: uint16) become the upper half of the float32 word
"""

import numpy as np

F32, F64, F16, BF16 = 0, 1, 2, 3
ELEM_BYTES = {F32: 4, F64: 8, F16: 2, BF16: 2}
STORAGE = {F32: np.float32, F64: np.float64, F16: np.float16, BF16: np.uint16}


def convert(raw, dtype):
  """Elements as they lie in memory (bfloat16: their uint16 bit patterns) -> float32."""
  raw = np.asarray(raw)
  assert raw.dtype == STORAGE[dtype], (raw.dtype, dtype)
  if dtype == BF16:
    return (raw.astype(np.uint32) << 16).view(np.float32)
  with np.errstate(over='ignore', invalid='ignore'):
    return raw.astype(np.float32)


def gather(blocks, dim):
  """blocks: dicts {storage, start, rows, row_stride, dtype} -> float32 [sum rows, dim]."""
  out = np.zeros((sum(b['rows'] for b in blocks), dim), dtype=np.float32)
  at = 0
  for b in blocks:
    for r in range(b['rows']):
      first = b['start'] + r * b['row_stride']
      out[at] = convert(b['storage'][first:first + dim], b['dtype'])
      at += 1
  return out


def refusal(blocks, dim, capacity_rows=None):
  """None, or why the library refuses the list (data: the block's address, 0 = NULL), in the order it checks."""
  for i, b in enumerate(blocks):
    if b['dtype'] not in ELEM_BYTES:
      return 'tensor {}: unknown dtype'.format(i)
    if b['rows'] < 0:
      return 'tensor {}: negative rows'.format(i)
    if b['rows'] == 0:
      continue
    if not b['data']:
      return 'tensor {}: rows but no data'.format(i)
    if b['row_stride'] < dim:
      return 'tensor {}: row_stride below observation_dim'.format(i)
    if b['data'] % ELEM_BYTES[b['dtype']]:
      return 'tensor {}: misaligned data'.format(i)
  if capacity_rows is not None and sum(b['rows'] for b in blocks) > capacity_rows:
    return 'capacity_rows too small'
  return None


def vector_flag(data, rows, row_stride, dtype, dim, out_address=0):
  """Whether the kernel may move the block 16 bytes at a time: every row's first element, and its place in the stream,
  must lie on a 16-byte boundary -- an aligned base is not enough where the row pitch misaligns every other row."""
  if rows == 0:
    return False
  esz = ELEM_BYTES[dtype]
  rows_in = all((data + r * row_stride * esz) % 16 == 0 for r in range(min(rows, 4)))
  rows_out = all((out_address + r * dim * 4) % 16 == 0 for r in range(4))
  # (a single-row block still needs the pitch: the rule is per block, decided without looking at its row count)
  return rows_in and rows_out and (row_stride * esz) % 16 == 0


def raw_values(tensor):
  """A torch tensor's elements (any device, any strides) as numpy in their storage type: [..., D]."""
  import torch  # pylint: disable=import-outside-toplevel
  t = tensor.detach().cpu().contiguous()
  if t.dtype == torch.bfloat16:
    return t.view(torch.int16).numpy().view(np.uint16)
  return t.numpy()


def code_of(tensor):
  import torch  # pylint: disable=import-outside-toplevel
  return {torch.float32: F32, torch.float64: F64, torch.float16: F16, torch.bfloat16: BF16}[tensor.dtype]


def expected(tensors, dim):
  """The packed stream of a list of [rows, D] torch tensors (None: no rows), from their VALUES."""
  parts = [convert(raw_values(t), code_of(t)).reshape(-1, dim) for t in tensors if t is not None]
  return np.concatenate(parts) if parts else np.zeros((0, dim), dtype=np.float32)
