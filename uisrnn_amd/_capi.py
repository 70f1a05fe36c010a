"""ctypes binding of the C ABI declared in include/uisrnn_hip.h.

The reference has no FFI; its boundary is the Python method set on
``uisrnn.UISRNN`` (uisrnn/__init__.py:26-30, uisrnn/uisrnn.py:479-623).  This
module is the thin layer between that Python surface (uisrnn_amd/uisrnn.py)
and ``libuisrnn_hip.so``.  There is deliberately NO fallback: if the HIP
library is missing or no gfx950 device is usable, the calls raise.
"""

import ctypes
import os
import struct
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libuisrnn_hip.so')

UIS_OK = 0
UIS_ABI_VERSION = 6   # include/uisrnn_hip.h
UIS_ERR_INVALID_ARG = -1
UIS_ERR_DIM_MISMATCH = -2
UIS_ERR_NO_DEVICE = -3
UIS_ERR_HIP = -4
UIS_ERR_OOM = -5
UIS_ERR_CLUSTER_CAP = -6
UIS_ERR_UNSUPPORTED = -7

UIS_FLAG_NO_DEDUP = 0x1
UIS_FLAG_GRAPH = 0x2
UIS_FLAG_PROFILE = 0x4
UIS_FLAG_GENERIC_SELECT = 0x8
UIS_FLAG_RESIDENT = 0x40
UIS_FLAG_STEPWISE = 0x80
UIS_FLAG_TEST_MISPLACED = 0x100
UIS_FLAG_TEST_STALL = 0x4000
UIS_FLAG_SMALL_TILES = 0x200
UIS_FLAG_PERSISTENT = 0x400
UIS_FLAG_OWNER_SELECT = 0x800
UIS_FLAG_REPLICATED_SELECT = 0x1000  # (reserved: the library ignores it)
UIS_FLAG_DEBUG_SCORES = 0x2000
UIS_FLAG_CLUSTER_BARRIERS = 0x8000
UIS_FLAG_COHORTS = 0x10000
UIS_FLAG_AGENT_FLAGS = 0x20000
UIS_BUILD_COHORTS = 0x1   # (reserved: uis_build_flags() never sets it)

UIS_N_KERNELS = 8
KERNEL_NAMES = ('input_proj', 'select', 'gru', 'head1', 'head2', 'backtrace',
                'upper_in', 'expand')

# uis_stats.decode_kernel (UIS_DK_* | UIS_DF_* << 8): the kernel family that ran the decode steps
DECODE_KERNELS = {0: 'none', 1: 'stepwise', 2: 'k_decode_rs', 3: 'k_decode_resident', 4: 'k_decode_big',
                  5: 'k_decode_big<WS>', 6: 'k_decode_small',
                  7: 'k_decode_big<WIN>', 8: 'k_decode_deep'}
DENSE_FAMILIES = {0: '', 1: 'k_dense', 2: 'k_big', 3: 'k_wt'}


def decode_kernel_name(code):
  name = DECODE_KERNELS.get(code & 0xff, 'unknown')
  fam = DENSE_FAMILIES.get((code >> 8) & 0xff, '')
  return name + (':' + fam if fam else '')


_fp = ctypes.POINTER(ctypes.c_float)
_fpp = ctypes.POINTER(_fp)
_i32p = ctypes.POINTER(ctypes.c_int32)
_i64p = ctypes.POINTER(ctypes.c_int64)


class ModelDesc(ctypes.Structure):
  """struct uis_model_desc (include/uisrnn_hip.h)."""
  _fields_ = [
      ('observation_dim', ctypes.c_int32),
      ('rnn_hidden_size', ctypes.c_int32),
      ('rnn_depth', ctypes.c_int32),
      ('reserved0', ctypes.c_int32),
      ('gru_weight_ih', _fpp),
      ('gru_weight_hh', _fpp),
      ('gru_bias_ih', _fpp),
      ('gru_bias_hh', _fpp),
      ('linear_mean1_weight', _fp),
      ('linear_mean1_bias', _fp),
      ('linear_mean2_weight', _fp),
      ('linear_mean2_bias', _fp),
      ('rnn_init_hidden', _fp),
      ('sigma2', _fp),
      ('transition_bias', ctypes.c_double),
      ('crp_alpha', ctypes.c_double),
  ]


class DecodeOpts(ctypes.Structure):
  """struct uis_decode_opts (include/uisrnn_hip.h)."""
  _fields_ = [
      ('beam_size', ctypes.c_int32),
      ('look_ahead', ctypes.c_int32),
      ('test_iteration', ctypes.c_int32),
      ('max_clusters', ctypes.c_int32),
      ('flags', ctypes.c_uint32),
      ('n_streams', ctypes.c_int32),
      ('level_cap', ctypes.c_int32),
      ('reserved', ctypes.c_int32 * 1),
  ]


class TrainOpts(ctypes.Structure):
  """struct uis_train_opts (include/uisrnn_hip.h)."""
  _fields_ = [
      ('learning_rate', ctypes.c_double),
      ('regularization_weight', ctypes.c_double),
      ('grad_max_norm', ctypes.c_double),
      ('sigma_alpha', ctypes.c_double),
      ('sigma_beta', ctypes.c_double),
      ('dropout', ctypes.c_double),
      ('dropout_key', ctypes.c_uint64),
      ('estimate_sigma2', ctypes.c_int32),
      ('reserved', ctypes.c_int32 * 3),
  ]


class Stats(ctypes.Structure):
  """struct uis_stats (include/uisrnn_hip.h)."""
  _fields_ = [
      ('n_steps', ctypes.c_int32),
      ('max_clusters_seen', ctypes.c_int32),
      ('rnn_rows', ctypes.c_int64),
      ('rnn_rows_nodedup', ctypes.c_int64),
      ('candidates', ctypes.c_int64),
      ('decode_ms', ctypes.c_double),
      ('kernel_ms', ctypes.c_double * UIS_N_KERNELS),
      ('kernel_launches', ctypes.c_int64 * UIS_N_KERNELS),
      ('n_overflow', ctypes.c_int32),
      ('n_streams', ctypes.c_int32),
      ('decode_kernel', ctypes.c_int32),
      ('decode_launches', ctypes.c_int32),
  ]

  def as_dict(self):
    return {
        'n_steps': self.n_steps,
        'max_clusters_seen': self.max_clusters_seen,
        'rnn_rows': self.rnn_rows,
        'rnn_rows_nodedup': self.rnn_rows_nodedup,
        'candidates': self.candidates,
        'decode_ms': self.decode_ms,
        'decode_launches': self.decode_launches,
        'kernel_ms': {n: self.kernel_ms[i] for i, n in enumerate(KERNEL_NAMES)},
        'kernel_launches': {
            n: self.kernel_launches[i] for i, n in enumerate(KERNEL_NAMES)},
        'n_overflow': self.n_overflow,
        'n_streams': self.n_streams,
        'decode_kernel': decode_kernel_name(self.decode_kernel),
        'decode_kernel_code': int(self.decode_kernel),   # the raw word: bits 16..23 = k_decode_rs's kind (1 generic, 2 the fixed-shape class)
    }


def _f32(a):
  return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _ptr(a):
  return a.ctypes.data_as(_fp)


def _i32(a):
  return a.ctypes.data_as(_i32p)


def _i64(a):
  return a.ctypes.data_as(_i64p)


def _offsets(counts):
  """int64 [U + 1]: where each utterance begins in a buffer packed by these counts, and where the last one ends."""
  return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


# ---- device tensors in (uis_ingest_tensors, uis_tensors_decode, uis_tensors_stream_push; csrc/uis_ingest.hip)

UIS_DTYPE_F32, UIS_DTYPE_F64, UIS_DTYPE_F16, UIS_DTYPE_BF16 = 0, 1, 2, 3
DTYPE_BYTES = {UIS_DTYPE_F32: 4, UIS_DTYPE_F64: 8, UIS_DTYPE_F16: 2, UIS_DTYPE_BF16: 2}
# struct uis_tensor, one record per block: a table is a numpy array of these, handed over by its address
TENSOR_RECORD = np.dtype([('data', np.uint64), ('rows', np.int64), ('row_stride', np.int64), ('dtype', np.int32),
                          ('reserved', np.int32)])
INGEST_WORKGROUP_ITEMS = 512   # items (8 consecutive floats of one row) a workgroup of k_ingest takes


def ingest_workgroup_rows(dim):
  """Rows of the packed stream one workgroup of k_ingest covers (the last one possibly in part)."""
  return INGEST_WORKGROUP_ITEMS // ((int(dim) + 7) // 8)


_dtype_codes = None   # {torch dtype: UIS_DTYPE_*}, made by the first tensor call (torch is imported no earlier)
_ELEM_BYTES = np.array([DTYPE_BYTES[c] for c in range(4)], dtype=np.int64)


def _torch_dtype_codes():
  global _dtype_codes
  if _dtype_codes is None:
    import torch  # pylint: disable=import-outside-toplevel
    _dtype_codes = {torch.float32: UIS_DTYPE_F32, torch.float64: UIS_DTYPE_F64, torch.float16: UIS_DTYPE_F16,
                    torch.bfloat16: UIS_DTYPE_BF16}
  return _dtype_codes


def _checked_tensor(t, ndim, dim, device, who):
  """One tensor of a tensor entry point, checked before the library is called: TypeError for what is no floating-point
  torch tensor on a GPU, ValueError for a wrong device index, rank or observation dimension.  device None: any device,
  the CPU included (descriptor building is plain arithmetic; the tests use it).  Returns (tensor, dtype code): the
  tensor itself, or a contiguous copy where its inner stride is not 1 or its rows overlap."""
  codes = _torch_dtype_codes()
  if type(t).__module__.split('.')[0] != 'torch' or not hasattr(t, 'data_ptr'):
    raise TypeError('{} should be a torch tensor, not {}.'.format(who, type(t).__name__))
  code = codes.get(t.dtype)
  if code is None:
    raise TypeError('{} should be of dtype float64, float32, float16 or bfloat16, not {}.'.format(who, t.dtype))
  if device is not None:
    if t.device.type != 'cuda':
      raise TypeError('{} is on the {}: tensors must be on the model\'s device (cuda:{}).'.format(who, t.device, device))
    if t.device.index != device:
      raise ValueError('{} is on {}, the model is on cuda:{}.'.format(who, t.device, device))
  if t.ndim != ndim:
    raise ValueError('{} must be a {}-dim tensor.'.format(who, ndim))
  if t.shape[-1] != dim:
    raise ValueError('{} does not match observation_dim ({} against {}).'.format(who, t.shape[-1], dim))
  rows_overlap = t.shape[-2] > 1 and t.stride(-2) < dim
  if (dim > 1 and t.stride(-1) != 1) or rows_overlap:
    t = t.contiguous()
  return t, code


def tensor_table(source, dim, lengths=None, device=None, who='test_sequences'):
  """The uis_tensor table of `source`: a list of [N_u, D] tensors (None: no rows), or one [U, T, D] tensor whose
  utterance u holds `lengths[u]` rows (None: T).  Returns (table, keep): a TENSOR_RECORD array with one record per
  utterance and whatever has to outlive the call that reads it.  A block of at most one row is given row_stride D
  where its own is smaller (a stride nothing is ever multiplied by)."""
  dim = int(dim)
  if hasattr(source, 'ndim') and not isinstance(source, (list, tuple)):
    batch, code = _checked_tensor(source, 3, dim, device, who)
    n_utt, most = int(batch.shape[0]), int(batch.shape[1])
    rows = np.full(n_utt, most, dtype=np.int64)
    if lengths is not None:
      rows = np.asarray(lengths.cpu() if hasattr(lengths, 'cpu') else lengths).astype(np.int64).reshape(-1)
      if rows.shape[0] != n_utt or (n_utt and (rows.min() < 0 or rows.max() > most)):
        raise ValueError('lengths must hold one value in [0, {}] per utterance.'.format(most))
    table = np.zeros(n_utt, dtype=TENSOR_RECORD)
    # (addresses lie below 2^63: int64 arithmetic)
    table['data'] = np.int64(batch.data_ptr()) + np.arange(n_utt, dtype=np.int64) * (int(batch.stride(0)) * DTYPE_BYTES[code])
    table['rows'] = rows
    table['row_stride'] = max(int(batch.stride(1)), dim) if most <= 1 else int(batch.stride(1))
    table['dtype'] = code
    return table, [batch]
  if lengths is not None:
    raise ValueError('lengths belongs to a [U, T, D] tensor.')
  table = np.zeros(len(source), dtype=TENSOR_RECORD)
  keep = []
  for u, t in enumerate(source):
    if t is None:
      table[u] = (0, 0, dim, UIS_DTYPE_F32, 0)
      continue
    t, code = _checked_tensor(t, 2, dim, device, '{}[{}]'.format(who, u))
    keep.append(t)
    rows = int(t.shape[0])
    table[u] = (t.data_ptr() if rows else 0, rows, max(int(t.stride(0)), dim) if rows <= 1 else int(t.stride(0)), code, 0)
  return table, keep


def check_tensor_table(table, dim, capacity_rows=None):
  """The library's checks of a uis_tensor list (uisrnn_hip.h), in its order, as ValueError: they hold before the
  library is called, whoever built the table."""
  codes, rows = table['dtype'], table['rows']
  if len(table) and ((codes >= 0) & (codes <= 3)).all():   # (the usual case in a few array operations: nothing to report)
    live, address = rows > 0, table['data'].view(np.int64)
    if not ((rows < 0) | (live & ((address == 0) | (table['row_stride'] < dim) | (address % _ELEM_BYTES[codes] != 0)))).any():
      total = int(rows.sum())
      if capacity_rows is None or total <= capacity_rows:
        return total
  for u, rec in enumerate(table):
    esz = DTYPE_BYTES.get(int(rec['dtype']))
    if esz is None:
      raise ValueError('tensor {} has an unknown dtype code {}.'.format(u, int(rec['dtype'])))
    if rec['rows'] < 0:
      raise ValueError('tensor {} has a negative row count.'.format(u))
    if rec['rows'] == 0:
      continue
    if not rec['data']:
      raise ValueError('tensor {} has rows but no data.'.format(u))
    if rec['row_stride'] < dim:
      raise ValueError('tensor {}: row_stride {} is below observation_dim {}.'.format(u, int(rec['row_stride']), dim))
    if int(rec['data']) % esz:
      raise ValueError('tensor {}: data is not aligned to its element size.'.format(u))
  total = int(table['rows'].sum()) if len(table) else 0
  if capacity_rows is not None and total > capacity_rows:
    raise ValueError('{} rows given, capacity_rows is {}.'.format(total, capacity_rows))
  return total


def tensor_vector_flags(table, dim, out_ptr=0):
  """Per block: whether k_ingest moves it with 16-byte loads and stores -- D a multiple of 4, the output base, the
  block's base and its row pitch in bytes all multiples of 16 (the rule of ingest_vec_ok in csrc/uis_ingest.hip)."""
  esz = np.array([DTYPE_BYTES[int(c)] for c in table['dtype']], dtype=np.int64)
  return ((dim % 4 == 0) & (int(out_ptr) % 16 == 0) & (table['data'].astype(np.int64) % 16 == 0) &
          ((table['row_stride'] * esz) % 16 == 0) & (table['rows'] > 0))


def _table_ptr(table):
  return ctypes.c_void_p(table.ctypes.data) if len(table) else None


def _cut(flat, offsets):
  """A packed buffer as one array (a copy) per utterance."""
  return [flat[offsets[u]:offsets[u + 1]].copy() for u in range(len(offsets) - 1)]


def make_desc(params):
  """Build a ModelDesc from a parameter dict (see uisrnn_amd/weights.py).

  Returns (desc, keepalive): keepalive holds the numpy buffers the struct
  points into and must outlive every use of desc.
  """
  depth = int(params['rnn_depth'])
  keep = []

  def arr(a, shape):
    a = _f32(a)
    if tuple(a.shape) != tuple(shape):
      raise ValueError('parameter has shape {} but {} is required'.format(
          a.shape, shape))
    keep.append(a)
    return a

  dim = int(params['observation_dim'])
  hid = int(params['rnn_hidden_size'])

  def ptr_array(key, shapes):
    arrs = [arr(params[key][l], shapes[l]) for l in range(depth)]
    pa = (_fp * depth)(*[_ptr(a) for a in arrs])
    keep.append(pa)
    return ctypes.cast(pa, _fpp)

  in_dims = [dim] + [hid] * (depth - 1)
  desc = ModelDesc()
  desc.observation_dim = dim
  desc.rnn_hidden_size = hid
  desc.rnn_depth = depth
  desc.gru_weight_ih = ptr_array(
      'gru_weight_ih', [(3 * hid, in_dims[l]) for l in range(depth)])
  desc.gru_weight_hh = ptr_array(
      'gru_weight_hh', [(3 * hid, hid)] * depth)
  desc.gru_bias_ih = ptr_array('gru_bias_ih', [(3 * hid,)] * depth)
  desc.gru_bias_hh = ptr_array('gru_bias_hh', [(3 * hid,)] * depth)
  desc.linear_mean1_weight = _ptr(arr(params['linear_mean1_weight'], (hid, hid)))
  desc.linear_mean1_bias = _ptr(arr(params['linear_mean1_bias'], (hid,)))
  desc.linear_mean2_weight = _ptr(arr(params['linear_mean2_weight'], (dim, hid)))
  desc.linear_mean2_bias = _ptr(arr(params['linear_mean2_bias'], (dim,)))
  desc.rnn_init_hidden = _ptr(arr(params['rnn_init_hidden'], (depth, hid)))
  desc.sigma2 = _ptr(arr(params['sigma2'], (dim,)))
  desc.transition_bias = float(params['transition_bias'])
  desc.crp_alpha = float(params['crp_alpha'])
  return desc, keep


def make_opts(beam_size, look_ahead, test_iteration, max_clusters=0, flags=0,
              n_streams=0, level_cap=0):
  opts = DecodeOpts()
  opts.level_cap = int(level_cap)
  opts.n_streams = int(n_streams)
  opts.beam_size = int(beam_size)
  opts.look_ahead = int(look_ahead)
  opts.test_iteration = int(test_iteration)
  opts.max_clusters = int(max_clusters)
  opts.flags = int(flags)
  return opts


class HipLibraryError(RuntimeError):
  """The HIP decoder library is missing, failed to load or reported an error."""
  status = None   # the uis_status of a failed call, where there was one


_lib = None
_hip_runtime = None   # what share_hip_runtime_with_torch() did, for whoever asks (tests, bench.py)


def share_hip_runtime_with_torch():
  """ONE HIP runtime per process, whichever of {this library, PyTorch} is loaded first (round 6).

  The PyTorch-ROCm wheel bundles its own libamdhip64.so (SONAME libamdhip64.so.7, the system ROCm's too).  With
  torch imported FIRST the dynamic linker resolves this library's `NEEDED libamdhip64.so.7` to torch's copy, already
  loaded under that SONAME: one runtime, everything works.  With this library first the system runtime is loaded, a
  later `import torch` brings a SECOND runtime (its NEEDED name is `libamdhip64.so`: no SONAME match) and
  torch.cuda.init() reports "No HIP GPUs are available" (measured, round 4).  So: where a torch installation is found
  and not yet imported, its libamdhip64.so is dlopen()ed (RTLD_GLOBAL, by path, WITHOUT importing torch) before this
  library -- both load orders then end in the first situation.  UIS_HIP_RUNTIME=system keeps the system runtime (for
  processes that never import torch)."""
  global _hip_runtime
  if _hip_runtime is not None:
    return _hip_runtime
  if os.environ.get('UIS_HIP_RUNTIME', 'auto') == 'system':
    _hip_runtime = 'system (UIS_HIP_RUNTIME)'
  elif 'torch' in sys.modules:
    _hip_runtime = 'torch (imported before this library)'
  else:
    _hip_runtime = 'system (no torch installation found)'
    try:
      import importlib.util  # pylint: disable=import-outside-toplevel
      spec = importlib.util.find_spec('torch')
      bundled = os.path.join(os.path.dirname(spec.origin), 'lib', 'libamdhip64.so') if spec and spec.origin else None
      if bundled and os.path.exists(bundled):
        ctypes.CDLL(bundled, mode=ctypes.RTLD_GLOBAL)
        _hip_runtime = 'torch (preloaded: ' + bundled + ')'
    except (ImportError, OSError, ValueError) as e:
      _hip_runtime = 'system (torch\'s runtime could not be preloaded: {})'.format(e)
  return _hip_runtime


def load_library(path=None):
  """dlopen libuisrnn_hip.so and declare every entry point of the header."""
  global _lib
  if _lib is not None and path is None:
    return _lib
  path = path or os.environ.get('UIS_LIB_PATH') or LIB_PATH
  if not os.path.exists(path):
    raise HipLibraryError(
        '{} not found: build it with `python -m uisrnn_amd.build` (hipcc, '
        'gfx950). There is no CPU fallback for the decode path.'.format(path))
  share_hip_runtime_with_torch()
  lib = ctypes.CDLL(path)
  lib.uis_abi_version.restype = ctypes.c_int32
  lib.uis_abi_version.argtypes = []
  if lib.uis_abi_version() != UIS_ABI_VERSION:
    # a stale in-tree build: its structs would not match the ctypes mirrors below
    raise HipLibraryError(
        '{} was built for ABI {} but this package expects {}: rebuild with '
        '`python -m uisrnn_amd.build --force`'.format(path, lib.uis_abi_version(), UIS_ABI_VERSION))
  i32 = ctypes.c_int32
  i32p, i64p = _i32p, _i64p
  lib.uis_abi_version.restype = i32
  lib.uis_abi_version.argtypes = []
  lib.uis_numerics_version.restype = i32
  lib.uis_numerics_version.argtypes = []
  lib.uis_build_flags.restype = ctypes.c_uint32
  lib.uis_build_flags.argtypes = []
  lib.uis_device_count.restype = i32
  lib.uis_device_count.argtypes = []
  lib.uis_create.restype = i32
  lib.uis_create.argtypes = [
      ctypes.POINTER(ModelDesc), i32, ctypes.POINTER(ctypes.c_void_p)]
  lib.uis_destroy.restype = None
  lib.uis_destroy.argtypes = [ctypes.c_void_p]
  lib.uis_decode.restype = i32
  lib.uis_decode.argtypes = [
      ctypes.c_void_p, _fp, i64p, i32, ctypes.POINTER(DecodeOpts), i32p, _fp,
      ctypes.POINTER(Stats)]
  lib.uis_decode_device.restype = i32
  lib.uis_decode_device.argtypes = [
      ctypes.c_void_p, ctypes.c_void_p, i64p, i32, ctypes.POINTER(DecodeOpts),
      ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Stats)]
  lib.uis_decode_f64.restype = i32
  lib.uis_decode_f64.argtypes = [
      ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), i64p, i32, ctypes.POINTER(DecodeOpts),
      i32p, _fp, ctypes.POINTER(Stats)]
  lib.uis_ingest_tensors.restype = i32
  lib.uis_ingest_tensors.argtypes = [ctypes.c_void_p, ctypes.c_void_p, i32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
  lib.uis_tensors_decode.restype = i32
  lib.uis_tensors_decode.argtypes = [
      ctypes.c_void_p, ctypes.c_void_p, i32, ctypes.c_void_p, ctypes.POINTER(DecodeOpts), ctypes.c_void_p, ctypes.c_void_p,
      ctypes.POINTER(Stats)]
  lib.uis_tensors_stream_push.restype = i32
  lib.uis_tensors_stream_push.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
  lib.uis_last_decode_info.restype = i32
  lib.uis_last_decode_info.argtypes = [ctypes.c_void_p, i32p, _fp]
  lib.uis_last_decode_shape.restype = i32
  lib.uis_last_decode_shape.argtypes = [ctypes.c_void_p, i32p, i32p]
  lib.uis_last_decode_instantiation.restype = i32
  lib.uis_last_decode_instantiation.argtypes = [ctypes.c_void_p, i32p]
  lib.uis_decode_kernel_table.restype = i32
  lib.uis_decode_kernel_table.argtypes = [i32p, i32]
  lib.uis_debug_scores.restype = i32
  lib.uis_debug_scores.argtypes = [ctypes.c_void_p, _fp, ctypes.c_int64]
  lib.uis_model_constants.restype = i32
  lib.uis_model_constants.argtypes = [ctypes.c_void_p, _fp, _fp]
  lib.uis_rnn_step.restype = i32
  lib.uis_rnn_step.argtypes = [ctypes.c_void_p, _fp, _fp, _fp, _fp]
  lib.uis_stream_begin.restype = i32
  lib.uis_stream_begin.argtypes = [ctypes.c_void_p, i32, ctypes.POINTER(DecodeOpts), ctypes.c_int64]
  lib.uis_stream_push.restype = i32
  lib.uis_stream_push.argtypes = [ctypes.c_void_p, _fp, i32p]
  lib.uis_stream_labels.restype = i32
  lib.uis_stream_labels.argtypes = [ctypes.c_void_p, i32p, _fp, i32p]
  lib.uis_stream_end.restype = i32
  lib.uis_stream_end.argtypes = [ctypes.c_void_p]
  lib.uis_decode_limits.restype = i32
  lib.uis_decode_limits.argtypes = [ctypes.c_void_p, i32p, i32]
  lib.uis_stream_limits.restype = i32
  lib.uis_stream_limits.argtypes = [ctypes.c_void_p, i32p]
  lib.uis_stream_get_limits.restype = i32
  lib.uis_stream_get_limits.argtypes = [ctypes.c_void_p, i32p]
  lib.uis_frame_bias.restype = i32
  lib.uis_frame_bias.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int64]
  lib.uis_frame_speakers.restype = i32
  lib.uis_frame_speakers.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int64]
  lib.uis_min_turn.restype = i32
  lib.uis_min_turn.argtypes = [ctypes.c_void_p, i32p, i32]
  lib.uis_session_min_turn.restype = i32
  lib.uis_session_min_turn.argtypes = [ctypes.c_void_p, i32p]
  lib.uis_session_get_min_turn.restype = i32
  lib.uis_session_get_min_turn.argtypes = [ctypes.c_void_p, i32p]
  lib.uis_session_turns.restype = i32
  lib.uis_session_turns.argtypes = [ctypes.c_void_p, i32p]
  lib.uis_stream_speakers.restype = i32
  lib.uis_stream_speakers.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int64]
  lib.uis_stream_bindings.restype = i32
  lib.uis_stream_bindings.argtypes = [ctypes.c_void_p, i32p]
  lib.uis_stream_prime.restype = i32
  lib.uis_stream_prime.argtypes = [ctypes.c_void_p, _fp, i64p, i32p, _fp]
  lib.uis_last_decode_nbest.restype = i32
  lib.uis_last_decode_nbest.argtypes = [ctypes.c_void_p, i32, i32p, ctypes.c_int64, _fp, i32p]
  lib.uis_stream_nbest.restype = i32
  lib.uis_stream_nbest.argtypes = [ctypes.c_void_p, i32, i32p, ctypes.c_int64, _fp, i32p, i64p]
  lib.uis_last_decode_posterior.restype = i32
  lib.uis_last_decode_posterior.argtypes = [ctypes.c_void_p, ctypes.c_double, _fp, _fp, ctypes.c_int64, _fp, i32p]
  lib.uis_stream_posterior.restype = i32
  lib.uis_stream_posterior.argtypes = [ctypes.c_void_p, ctypes.c_double, _fp, _fp, ctypes.c_int64, _fp, i32p]
  lib.uis_stream_commit.restype = i32
  lib.uis_stream_commit.argtypes = [ctypes.c_void_p, i32p, i32p, ctypes.c_int64, i32p, i32p]
  lib.uis_stream_committed.restype = i32
  lib.uis_stream_committed.argtypes = [ctypes.c_void_p, i64p]
  lib.uis_stream_restart.restype = i32
  lib.uis_stream_restart.argtypes = [ctypes.c_void_p, i32p, i32p, ctypes.c_int64, i32p, _fp, i32p]
  lib.uis_stream_retire.restype = i32
  lib.uis_stream_retire.argtypes = [ctypes.c_void_p, i32p, i64p, i32p, i32p, i32p, i32p, i32p, i32p]
  lib.uis_stream_export_bound.restype = i32
  lib.uis_stream_export_bound.argtypes = [ctypes.c_void_p, i32, i64p]
  lib.uis_stream_export.restype = i32
  lib.uis_stream_export.argtypes = [ctypes.c_void_p, i32, ctypes.c_void_p, ctypes.c_int64, i64p]
  lib.uis_stream_import.restype = i32
  lib.uis_stream_import.argtypes = [ctypes.c_void_p, i32, ctypes.c_void_p, ctypes.c_int64]
  lib.uis_eval_accuracy.restype = i32
  lib.uis_eval_accuracy.argtypes = [ctypes.c_void_p, i32p, i32p, i64p, i32, i64p]
  lib.uis_eval_accuracy_device.restype = i32
  lib.uis_eval_accuracy_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, i64p, i32, i64p]
  lib.uis_score_labels.restype = i32
  lib.uis_score_labels.argtypes = [ctypes.c_void_p, _fp, i64p, i32, i32p, _fp, _fp]
  lib.uis_score_speakers.restype = i32
  lib.uis_score_speakers.argtypes = [ctypes.c_void_p, _fp, i64p, i32, i32p, i32, _fp, _fp]
  lib.uis_speaker_profiles.restype = i32
  lib.uis_speaker_profiles.argtypes = [ctypes.c_void_p, _fp, i64p, i32, i32p, i32, i32p, i32p, _fp, _fp, _fp, _fp]
  lib.uis_session_profiles.restype = i32
  lib.uis_session_profiles.argtypes = [ctypes.c_void_p, i32, i32p, i32p, _fp]
  lib.uis_eval_last_decode.restype = i32
  lib.uis_eval_last_decode.argtypes = [ctypes.c_void_p, i32p, i32, i64p]
  lib.uis_host_alloc.restype = i32
  lib.uis_host_alloc.argtypes = [ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
  lib.uis_host_free.restype = None
  lib.uis_host_free.argtypes = [ctypes.c_void_p]
  lib.uis_last_error.restype = ctypes.c_char_p
  lib.uis_last_error.argtypes = []
  lib.uis_train_create.restype = i32
  lib.uis_train_create.argtypes = [
      ctypes.POINTER(ModelDesc), ctypes.POINTER(TrainOpts), i32, ctypes.POINTER(ctypes.c_void_p)]
  lib.uis_train_set_data.restype = i32
  lib.uis_train_set_data.argtypes = [ctypes.c_void_p, _fp, i64p, i32]
  lib.uis_train_step.restype = i32
  lib.uis_train_step.argtypes = [ctypes.c_void_p, i32p, i32, _fp]
  lib.uis_train_param_count.restype = i32
  lib.uis_train_param_count.argtypes = [ctypes.c_void_p, i64p]
  lib.uis_train_get_params.restype = i32
  lib.uis_train_get_params.argtypes = [ctypes.c_void_p, _fp, ctypes.c_int64]
  lib.uis_train_get_grads.restype = i32
  lib.uis_train_get_grads.argtypes = [ctypes.c_void_p, _fp, ctypes.c_int64]
  lib.uis_train_destroy.restype = None
  lib.uis_train_destroy.argtypes = [ctypes.c_void_p]
  _lib = lib
  return lib


EXPORTED_SYMBOLS = (
    'uis_abi_version', 'uis_numerics_version', 'uis_build_flags', 'uis_device_count', 'uis_create', 'uis_destroy',
    'uis_decode', 'uis_decode_f64', 'uis_decode_device', 'uis_last_decode_info', 'uis_last_decode_shape',
    'uis_last_decode_instantiation', 'uis_decode_kernel_table', 'uis_debug_scores',
    'uis_model_constants', 'uis_rnn_step', 'uis_stream_begin', 'uis_stream_push',
    'uis_stream_labels', 'uis_stream_end', 'uis_stream_prime', 'uis_last_decode_nbest', 'uis_stream_nbest', 'uis_last_decode_posterior', 'uis_stream_posterior', 'uis_stream_commit', 'uis_stream_committed', 'uis_stream_restart', 'uis_stream_retire',
    'uis_stream_export_bound', 'uis_stream_export', 'uis_stream_import', 'uis_eval_accuracy', 'uis_eval_accuracy_device',
    'uis_eval_last_decode', 'uis_score_labels', 'uis_score_speakers', 'uis_decode_limits', 'uis_stream_limits',
    'uis_stream_get_limits', 'uis_frame_bias', 'uis_frame_speakers', 'uis_min_turn', 'uis_stream_speakers', 'uis_stream_bindings',
    'uis_session_min_turn', 'uis_session_get_min_turn', 'uis_session_turns',
    'uis_speaker_profiles', 'uis_session_profiles',
    'uis_ingest_tensors', 'uis_tensors_decode', 'uis_tensors_stream_push',
    'uis_host_alloc', 'uis_host_free', 'uis_last_error',
    'uis_train_create', 'uis_train_set_data', 'uis_train_step', 'uis_train_param_count',
    'uis_train_get_params', 'uis_train_get_grads', 'uis_train_destroy')


_BLOB_HEAD = struct.Struct('<4I8iQq' 'q4ifi')   # UisBlobHeader, UisBlobScalars (csrc/uis_blob.h)
BLOB_MAGIC = 0x42534955


def blob_info(blob):
  """The scalars of a uis_stream_export blob: dict(B, N, committed, live, slots, K, bytes) -- K the largest cluster
  count over its live hypotheses.  ValueError for bytes that are no such blob (only the head is looked at: the
  library's import validates everything)."""
  if len(blob) < _BLOB_HEAD.size + 16:
    raise ValueError('not a stream blob: too short')
  f = _BLOB_HEAD.unpack_from(blob, 0)
  if f[0] != BLOB_MAGIC:
    raise ValueError('not a stream blob: bad magic')
  live = f[16]
  if not 0 <= live <= 256 or len(blob) < _BLOB_HEAD.size + 16 * live:
    raise ValueError('not a stream blob: bad live count')
  ks = [struct.unpack_from('<i', blob, _BLOB_HEAD.size + 16 * r)[0] for r in range(live)]
  return {'B': f[4], 'bytes': f[13], 'committed': f[14], 'N': f[15], 'live': live, 'slots': f[17], 'K': max(ks, default=0)}


def blob_max_tag(blob):
  """The largest speaker tag (bits 24 .. 30 of a block-count word, csrc/uis_blob.h) any live hypothesis of a
  uis_stream_export blob has bound; 0: the blob carries none.  From the blob's bytes alone; ValueError as blob_info's.
  Bytes that end inside the lists give 0: the library's import validates everything, and refuses them."""
  info = blob_info(blob)
  at = _BLOB_HEAD.size + 16 * info['live']   # the lists: rank by rank, K slot indices, then K block-count words
  most = 0
  for r in range(info['live']):
    k = struct.unpack_from('<i', blob, _BLOB_HEAD.size + 16 * r)[0]
    if k < 0 or at + 8 * k > len(blob):
      return 0
    if k:
      most = max(most, max(w >> 24 for w in struct.unpack_from('<{}i'.format(k), blob, at + 4 * k)))
    at += 8 * k
  return most


def decode_kernel_table(lib=None):
  """Every instantiation of the one-launch decode kernels, from the library's own tables (no device needed): a list of
  (family, Hp, Dp, variant, persist) -- family a name of DECODE_KERNELS."""
  lib = lib or load_library()
  n = lib.uis_decode_kernel_table(None, 0)
  rows = np.zeros((n, 5), dtype=np.int32)
  lib.uis_decode_kernel_table(_i32(rows), n)
  return [(DECODE_KERNELS.get(int(r[0]), 'unknown'),) + tuple(int(v) for v in r[1:]) for r in rows]


def last_error(lib):
  msg = lib.uis_last_error()
  return msg.decode('utf-8', 'replace') if msg else ''


def _raise_status(lib, rc, what):
  """The failed call `what` as an exception: ValueError for UIS_ERR_DIM_MISMATCH, else HipLibraryError with .status."""
  msg = last_error(lib)
  if rc == UIS_ERR_DIM_MISMATCH:
    raise ValueError(msg)
  err = HipLibraryError('{} failed ({}): {}'.format(what, rc, msg))
  err.status = rc
  raise err


class Decoder:
  """Owns one uis_handle (one HIP device)."""

  def __init__(self, params, device=0):
    self._lib = load_library()
    self.params = params
    self.observation_dim = int(params['observation_dim'])
    desc, keep = make_desc(params)
    handle = ctypes.c_void_p()
    rc = self._lib.uis_create(ctypes.byref(desc), int(device),
                              ctypes.byref(handle))
    del keep
    if rc != UIS_OK:
      raise HipLibraryError('uis_create failed ({}): {}'.format(
          rc, last_error(self._lib)))
    self._handle = handle
    self.device = int(device)
    self._last_offsets = None  # offsets of the last decode through this object: last_nbest() sizes its buffers from them
    self._export_buf = None    # stream_export's landing buffer (grow only)

  def close(self):
    if getattr(self, '_handle', None):
      self._lib.uis_destroy(self._handle)
      self._handle = None

  def __del__(self):
    try:
      self.close()
    except Exception:  # pylint: disable=broad-except
      pass

  def constants(self):
    """(m0 [D], h1 [depth, H]) as computed on the device at create time."""
    m0 = np.empty(self.observation_dim, dtype=np.float32)
    h1 = np.empty((int(self.params['rnn_depth']),
                   int(self.params['rnn_hidden_size'])), dtype=np.float32)
    self._check(self._lib.uis_model_constants(
        self._handle, m0.ctypes.data_as(_fp), h1.ctypes.data_as(_fp)),
                'uis_model_constants')
    return m0, h1

  def rnn_step(self, x, h_in):
    """CoreRNN.forward of one row on the device: x [D], h_in [depth, H]."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    h_in = np.ascontiguousarray(h_in, dtype=np.float32)
    mean = np.empty(self.observation_dim, dtype=np.float32)
    h_out = np.empty_like(h_in)
    self._check(self._lib.uis_rnn_step(
        self._handle, x.ctypes.data_as(_fp), h_in.ctypes.data_as(_fp),
        mean.ctypes.data_as(_fp), h_out.ctypes.data_as(_fp)), 'uis_rnn_step')
    return mean, h_out

  def _check(self, rc, what, ok=(UIS_OK, UIS_ERR_CLUSTER_CAP)):
    """rc if it is one of `ok`, else the exception.  UIS_ERR_CLUSTER_CAP is a result with per-utterance flags for the
    calls that decode or read out; the calls for which it is a refusal pass ok=(UIS_OK,)."""
    if rc in ok:
      return rc
    _raise_status(self._lib, rc, what)

  def _set_table(self, what, values, convert):
    """One per-call table of the library (uis_call_tables.h) through the setter named `what`: None clears, else the
    array `convert` makes of `values` is handed over with its first dimension as the length."""
    call = getattr(self._lib, what)
    if values is None:
      self._check(call(self._handle, None, 0), what)
      return
    arr = convert(values)
    self._check(call(self._handle, arr.ctypes.data_as(call.argtypes[1]), int(arr.shape[0])), what)

  @staticmethod
  def _tags(speakers):
    tags = np.asarray(speakers).reshape(-1)
    if tags.size and (tags.min() < 0 or tags.max() > 255):
      raise ValueError('speaker tags must lie in 0 .. 127')
    return np.ascontiguousarray(tags, dtype=np.uint8)

  def set_limits(self, limits):
    """uis_decode_limits: the max_speakers table (ints, 0 = no bound; None clears) of the NEXT decode* /
    stream_begin call on this decoder, which consumes it."""
    self._set_table('uis_decode_limits', limits, lambda v: np.ascontiguousarray(v, dtype=np.int32))

  def set_frame_bias(self, bias):
    """uis_frame_bias: the per-frame transition_bias (float64, one value per frame in the call's frame order, NaN = the
    model's; None clears) of the NEXT decode* / stream_push / score_* call on this decoder, which consumes it."""
    self._set_table('uis_frame_bias', bias, lambda v: np.ascontiguousarray(v, dtype=np.float64).reshape(-1))

  def set_frame_speakers(self, speakers):
    """uis_frame_speakers: the known speakers (uint8, one tag per frame in the call's frame order, 0 = unknown, 1 .. 127
    a speaker; None clears) of the NEXT decode* call on this decoder, which consumes it."""
    self._set_table('uis_frame_speakers', speakers, self._tags)

  def set_min_turn(self, min_turn):
    """uis_min_turn: the minimum turn lengths (ints, one per utterance, 0 and 1 = no rule; None clears) of the NEXT
    decode* call on this decoder, which consumes it."""
    self._set_table('uis_min_turn', min_turn, lambda v: np.ascontiguousarray(v, dtype=np.int32).reshape(-1))

  def set_stream_speakers(self, speakers):
    """uis_stream_speakers: the known speakers (uint8, one tag per frame in the call's own frame order, 0 = unknown,
    1 .. 127 a speaker; None clears) of the NEXT stream_push / stream_prime on this decoder, which consumes it."""
    self._set_table('uis_stream_speakers', speakers, self._tags)

  def _packed(self, frames, offsets, labels=None):
    """Packed utterances, checked: float32 frames [sum N, D], int64 offsets [U + 1] and, if given, int32 labels
    [sum N]."""
    frames = np.ascontiguousarray(frames, dtype=np.float32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    if labels is not None:
      labels = np.ascontiguousarray(labels, dtype=np.int32)
    total = int(offsets[-1])
    if frames.ndim != 2 or frames.shape[0] != total:
      raise ValueError('frames must be [offsets[-1], D]')
    if total and frames.shape[1] != self.observation_dim:
      raise ValueError('frames do not match observation_dim')
    if labels is not None and labels.shape != (total,):
      raise ValueError('labels must be [offsets[-1]]')
    return frames, offsets, labels

  def _run_decode(self, call, what, opts, frames, counts, offsets, labels, scores, limits, bias, speakers=None,
                  min_turn=None):
    """One decode call of the library -- uis_decode, uis_decode_f64 and uis_decode_device take the same arguments in
    the same places: `frames`, `labels` and `scores` as ctypes passes them on, `counts` the int64 array in third place
    (the offsets; the lengths for uis_decode_f64).  `offsets` is kept, as it is, as the layout of this decode, for
    last_nbest and last_posterior: an array the caller of the wrapper may still write to comes as a copy.  Returns
    {'stats', 'status'}."""
    stats = Stats()
    # the tables are those of the NEXT call on the handle, which consumes them: limits, bias, speakers, min_turn, the
    # decode -- nothing between
    if limits is not None:
      self.set_limits(limits)
    if bias is not None:
      self.set_frame_bias(bias)
    if speakers is not None:
      self.set_frame_speakers(speakers)
    if min_turn is not None:
      self.set_min_turn(min_turn)
    rc = self._check(call(self._handle, frames, _i64(counts), offsets.shape[0] - 1, ctypes.byref(opts), labels, scores,
                          ctypes.byref(stats)), what)
    self._last_offsets = offsets
    return {'stats': stats.as_dict(), 'status': rc}

  def _with_decode_info(self, out, n_utt, beam_size, want_beam_scores):
    """decode()'s dict with the overflow words (and the beam's scores) of the decode just made (uis_last_decode_info)."""
    out['overflow'] = np.zeros(n_utt, dtype=np.int32)
    if want_beam_scores:
      out['beam_scores'] = np.empty((n_utt, int(beam_size)), dtype=np.float32)
    self._check(self._lib.uis_last_decode_info(
        self._handle, _i32(out['overflow']), _ptr(out['beam_scores']) if want_beam_scores else None),
                'uis_last_decode_info')
    return out

  def decode(self, frames, offsets, beam_size, look_ahead, test_iteration,
             max_clusters=0, flags=0, want_beam_scores=False, n_streams=0, level_cap=0, limits=None, bias=None, speakers=None,
             min_turn=None):
    """Decode packed host utterances.

    Args:
      frames: float32 [sum N, D] C-contiguous.
      offsets: int64 [U + 1].
    Returns:
      dict with labels (int32 [sum N]), scores (float32 [U]), overflow
      (int32 [U]), stats (dict) and optionally beam_scores [U, beam_size].
    """
    frames, offsets, _ = self._packed(frames, offsets)
    n_utt = offsets.shape[0] - 1
    labels = np.empty(int(offsets[-1]), dtype=np.int32)
    scores = np.empty(n_utt, dtype=np.float32)
    opts = make_opts(beam_size, look_ahead, test_iteration, max_clusters, flags, n_streams, level_cap)
    out = self._run_decode(self._lib.uis_decode, 'uis_decode', opts, _ptr(frames), offsets, offsets.copy(),
                           _i32(labels), _ptr(scores), limits, bias, speakers, min_turn)
    out.update(labels=labels, scores=scores)
    return self._with_decode_info(out, n_utt, beam_size, want_beam_scores)

  def decode_f64(self, sequences, beam_size, look_ahead, test_iteration,
                 max_clusters=0, flags=0, want_beam_scores=False, n_streams=0, level_cap=0, limits=None, bias=None, speakers=None,
                 min_turn=None):
    """Decode a list of [N_u, D] float64 arrays as predict() receives them (uis_decode_f64:
    the library casts to float32 on its own threads while earlier chunks travel to the device).

    Returns the dict of decode(); labels are packed in utterance order.
    """
    seqs = [np.ascontiguousarray(s, dtype=np.float64) for s in sequences]  # (no copy when already so)
    n_utt = len(seqs)
    for s in seqs:
      if s.ndim != 2 or (s.shape[0] and s.shape[1] != self.observation_dim):
        raise ValueError('frames do not match observation_dim')
    lens = np.array([s.shape[0] for s in seqs], dtype=np.int64)
    offsets = _offsets(lens)
    ptrs = (ctypes.c_void_p * max(n_utt, 1))(*[s.ctypes.data if s.shape[0] else None for s in seqs])
    labels = np.empty(int(offsets[-1]), dtype=np.int32)
    scores = np.empty(n_utt, dtype=np.float32)
    opts = make_opts(beam_size, look_ahead, test_iteration, max_clusters, flags, n_streams, level_cap)
    out = self._run_decode(self._lib.uis_decode_f64, 'uis_decode_f64', opts, ptrs, lens, offsets,
                           _i32(labels), _ptr(scores), limits, bias, speakers, min_turn)
    out.update(labels=labels, scores=scores)
    return self._with_decode_info(out, n_utt, beam_size, want_beam_scores)

  def score_labels(self, frames, offsets, labels, want_frame_losses=False, bias=None):
    """The model's NLL of given labelings (uis_score_labels).

    Args:
      frames: float32 [sum N, D]; offsets: int64 [U + 1], packed as for decode().
      labels: int [sum N] in first-appearance form per utterance.
    Returns:
      float32 scores [U], and with want_frame_losses also the float32 per-frame losses [sum N].
    """
    frames, offsets, labels = self._packed(frames, offsets, labels)
    n_utt = offsets.shape[0] - 1
    scores = np.empty(n_utt, dtype=np.float32)
    losses = np.empty(int(offsets[-1]), dtype=np.float32) if want_frame_losses else None
    if bias is not None:
      self.set_frame_bias(bias)
    rc = self._lib.uis_score_labels(
        self._handle, _ptr(frames), _i64(offsets), n_utt, _i32(labels), _ptr(scores),
        _ptr(losses) if want_frame_losses else None)
    self._check(rc, 'uis_score_labels')
    return (scores, losses) if want_frame_losses else scores

  def score_speakers(self, frames, offsets, labels, width, losses_out=None, bias=None):
    """Every speaker's per-frame loss along given labelings (uis_score_speakers).

    Args:
      frames, offsets, labels: as score_labels.
      width: columns per row: at least the largest cluster count of the utterances + 1.
      losses_out: a C-contiguous float32 [sum N, width] array to fill instead of a new one (pinned memory, say: at a
        million frames the copy of the rows into pageable memory is the larger part of what the call adds).
    Returns:
      (float32 scores [U] -- score_labels' bits --, float32 losses [sum N, width]): losses[t, k] is the step loss of
      assigning frame t to its utterance's cluster k given the labels before t, column K(t) the new-speaker candidate,
      +inf past it and everywhere after an invalid label.
    """
    frames, offsets, labels = self._packed(frames, offsets, labels)
    n_utt = offsets.shape[0] - 1
    total = int(offsets[-1])
    width = int(width)
    scores = np.empty(n_utt, dtype=np.float32)
    losses = np.empty((total, max(width, 0)), dtype=np.float32) if losses_out is None else losses_out
    if losses.dtype != np.float32 or losses.shape != (total, max(width, 0)) or not losses.flags['C_CONTIGUOUS']:
      raise ValueError('losses_out must be a C-contiguous float32 [offsets[-1], width] array')
    if bias is not None:
      self.set_frame_bias(bias)
    rc = self._lib.uis_score_speakers(
        self._handle, _ptr(frames), _i64(offsets), n_utt, _i32(labels), width, _ptr(losses), _ptr(scores))
    self._check(rc, 'uis_score_speakers')
    return scores, losses

  def speaker_profiles(self, frames, offsets, labels, width, bias=None):
    """The speakers of given labelings (uis_speaker_profiles).

    Args:
      frames, offsets, labels: as score_labels.
      width: rows per utterance: at least the largest cluster count of the utterances.
      bias: a per-frame transition_bias table; it reaches `scores` only.
    Returns:
      dict(n_clusters int32 [U] (-1: an invalid trace), stats int32 [U, width, 4] {frames, blocks, first, last},
      mean / sum_x / sum_r2 float32 [U, width, D], scores float32 [U] -- score_labels' bits).  Rows past an utterance's
      cluster count, and every row of an invalid trace: stats {0, 0, -1, -1} and +0.0.
    """
    frames, offsets, labels = self._packed(frames, offsets, labels)
    n_utt = offsets.shape[0] - 1
    width = int(width)
    rows = (n_utt, max(width, 0))
    dim = self.observation_dim
    out = {'n_clusters': np.zeros(n_utt, dtype=np.int32), 'stats': np.zeros(rows + (4,), dtype=np.int32),
           'mean': np.zeros(rows + (dim,), dtype=np.float32), 'sum_x': np.zeros(rows + (dim,), dtype=np.float32),
           'sum_r2': np.zeros(rows + (dim,), dtype=np.float32), 'scores': np.zeros(n_utt, dtype=np.float32)}
    if bias is not None:
      self.set_frame_bias(bias)
    rc = self._lib.uis_speaker_profiles(
        self._handle, _ptr(frames), _i64(offsets), n_utt, _i32(labels), width, _i32(out['n_clusters']), _i32(out['stats']),
        _ptr(out['mean']), _ptr(out['sum_x']), _ptr(out['sum_r2']), _ptr(out['scores']))
    self._check(rc, 'uis_speaker_profiles')
    return out

  def last_instantiation(self):
    """(family, Hp, Dp, variant, persist) of the kernel-table entry behind the last decode, or behind the last
    launch of a stream_push: uis_last_decode_instantiation, family as a name of DECODE_KERNELS."""
    out = (ctypes.c_int32 * 5)()
    self._check(self._lib.uis_last_decode_instantiation(self._handle, out), 'uis_last_decode_instantiation')
    return (DECODE_KERNELS.get(int(out[0]), 'unknown'),) + tuple(int(v) for v in out[1:])

  def last_overflow(self, n_utt=None):
    """Per-utterance flags of the last decode: bit 0 = a survivor hit the cluster cap, bit 1 = an
    intermediate level of a look-ahead window was full (uis_last_decode_info).

    The buffer is sized from the library (uis_last_decode_shape), never from the caller's idea of
    the batch: a decode that was refused before it started leaves zero utterances behind, and the
    result is then an empty array.  `n_utt`, if given, only pads / cuts the returned array."""
    n_lib, beam = ctypes.c_int32(0), ctypes.c_int32(0)
    self._check(self._lib.uis_last_decode_shape(self._handle, ctypes.byref(n_lib), ctypes.byref(beam)),
                'uis_last_decode_shape')
    overflow = np.zeros(max(int(n_lib.value), 1), dtype=np.int32)
    self._check(self._lib.uis_last_decode_info(self._handle, _i32(overflow), None), 'uis_last_decode_info')
    overflow = overflow[:int(n_lib.value)]
    if n_utt is not None and int(n_utt) != overflow.shape[0]:
      padded = np.zeros(int(n_utt), dtype=np.int32)
      padded[:min(int(n_utt), overflow.shape[0])] = overflow[:int(n_utt)]
      return padded
    return overflow

  def debug_scores(self, n_windows, n_utt, beam_size, max_clusters, look_ahead=1):
    """The candidate scores of the last decode (flags included UIS_FLAG_DEBUG_SCORES):
    float32 [n_windows, n_utt, beam_size] + [max_clusters + 1] * look_ahead, +inf where
    _calculate_score's padded array (uisrnn/uisrnn.py:534-545) holds +inf.  n_windows =
    ceil(test_iteration * longest utterance / look_ahead)."""
    out = np.empty([int(n_windows), int(n_utt), int(beam_size)] + [int(max_clusters) + 1] * int(look_ahead),
                   dtype=np.float32)
    self._check(self._lib.uis_debug_scores(self._handle, out.ctypes.data_as(_fp), out.size), 'uis_debug_scores')
    return out

  # ---- online decoding (uis_stream_*)
  def stream_begin(self, n_utt, beam_size, max_frames, max_clusters=0, flags=0, limits=None):
    """Open a streaming session for n_utt utterances (test_iteration 1, look_ahead 1); `limits`: the slots'
    max_speakers (ints, 0 = no bound)."""
    opts = make_opts(beam_size, 1, 1, max_clusters, flags, 0)
    if limits is not None:
      self.set_limits(limits)
    rc = self._lib.uis_stream_begin(self._handle, int(n_utt), ctypes.byref(opts), int(max_frames))
    self._check(rc, 'uis_stream_begin')
    self._stream_n = int(n_utt)
    self._stream_beam = int(beam_size)
    self._stream_cap = int(max_clusters) if int(max_clusters) > 0 else 16
    self._stream_have = np.zeros(int(n_utt), dtype=np.int64)
    self._stream_counts = np.zeros(int(n_utt), dtype=np.int32)   # (reused by every push: its pointer is bound once)
    self._stream_counts_ptr = self._stream_counts.ctypes.data_as(_i32p)

  def stream_set_limits(self, limits):
    """uis_stream_limits: replace the open session's max_speakers table (one int per slot, 0 = no bound)."""
    lim = np.ascontiguousarray(limits, dtype=np.int32)
    if lim.shape != (self._stream_n,):
      raise ValueError('one limit per utterance of the session')
    self._check(self._lib.uis_stream_limits(self._handle, _i32(lim)), 'uis_stream_limits')

  def stream_limits(self):
    """uis_stream_get_limits: int32 [n_utt], 0 = no bound."""
    out = np.zeros(self._stream_n, dtype=np.int32)
    self._check(self._lib.uis_stream_get_limits(self._handle, _i32(out)), 'uis_stream_get_limits')
    return out

  def session_set_min_turn(self, min_turn):
    """uis_session_min_turn: replace the open session's minimum turn lengths (one int per slot, 0 and 1 = no rule).  A
    slot that has received frames keeps its value: HipLibraryError (UIS_ERR_INVALID_ARG) and nothing changes."""
    turns = np.ascontiguousarray(min_turn, dtype=np.int32)
    if turns.shape != (self._stream_n,):
      raise ValueError('one minimum turn length per utterance of the session')
    self._check(self._lib.uis_session_min_turn(self._handle, _i32(turns)), 'uis_session_min_turn')

  def session_min_turn(self):
    """uis_session_get_min_turn: int32 [n_utt], 0 and 1 = no rule."""
    out = np.zeros(self._stream_n, dtype=np.int32)
    self._check(self._lib.uis_session_get_min_turn(self._handle, _i32(out)), 'uis_session_get_min_turn')
    return out

  def session_turns(self):
    """uis_session_turns: int32 [n_utt, 2] -- {the best hypothesis' last label in the numbering of stream_labels at this
    moment, its run}; the run is 0 where the slot has no rule; {-1, 0} without a live hypothesis."""
    out = np.zeros((self._stream_n, 2), dtype=np.int32)
    self._check(self._lib.uis_session_turns(self._handle, _i32(out)), 'uis_session_turns', ok=(UIS_OK,))
    return out

  def stream_profiles(self, width=None):
    """uis_session_profiles: the speakers of each utterance's best hypothesis right now -- dict(n_clusters int32 [U]
    (0: nothing received, -1: no live hypothesis), stats int32 [U, width, 4] {frames, blocks, tag, 0}, mean float32
    [U, width, D]); cluster indices in the numbering of stream_labels at this moment; rows past the cluster count hold
    {0, 0, -1, -1} and +0.0.  width defaults to the session's max_clusters and may not be smaller."""
    width = self._stream_cap if width is None else int(width)
    rows = (self._stream_n, max(width, 0))
    out = {'n_clusters': np.zeros(self._stream_n, dtype=np.int32), 'stats': np.zeros(rows + (4,), dtype=np.int32),
           'mean': np.zeros(rows + (self.observation_dim,), dtype=np.float32)}
    rc = self._lib.uis_session_profiles(self._handle, width, _i32(out['n_clusters']), _i32(out['stats']), _ptr(out['mean']))
    self._check(rc, 'uis_session_profiles', ok=(UIS_OK,))
    return out

  def stream_push(self, chunks, bias=None, speakers=None):
    """chunks: one [n_u, D] array (or None / empty) per utterance: its new frames -- or ONE
    [n_utt, n, D] array when every utterance has the same number of new frames (one cast, no
    per-utterance Python work: the low-latency way to feed a live session).  bias: this push's per-frame
    transition_bias, float64 in the chunk's own frame order (utterance-major), or None (set_frame_bias).  speakers:
    this push's tags, uint8 in the same order, or None (set_stream_speakers)."""
    if len(chunks) != self._stream_n:
      raise ValueError('one chunk (or None) per utterance')
    dim = self.observation_dim
    if isinstance(chunks, np.ndarray) and chunks.ndim == 3:
      if chunks.shape[2] != dim:
        raise ValueError('chunk does not match observation_dim')
      frames = np.ascontiguousarray(chunks, dtype=np.float32)
      counts = np.full(self._stream_n, chunks.shape[1], dtype=np.int32)
      if bias is not None:
        self.set_frame_bias(bias)
      if speakers is not None:
        self.set_stream_speakers(speakers)
      rc = self._lib.uis_stream_push(
          self._handle, frames.ctypes.data_as(_fp) if frames.size else None,
          counts.ctypes.data_as(_i32p))
      self._check(rc, 'uis_stream_push')
      self._stream_have += counts
      return
    # (round 6) the list form without per-chunk numpy work: ONE concatenate over the caller's arrays (it checks that
    # they are 2-dimensional and of one width), one cast, the counts written into a buffer whose ctypes pointer was
    # made when the session opened -- a one-frame push of 64 utterances spent 56 us here, against 44 us in the library
    counts = self._stream_counts
    try:
      counts[:] = [c.shape[0] for c in chunks]   # (a None entry has no shape: the careful path below)
      frames64 = np.concatenate(chunks)
      if frames64.ndim != 2 or frames64.dtype != np.float64 or len({c.dtype for c in chunks}) != 1:
        raise TypeError
    except (TypeError, ValueError, AttributeError, IndexError):
      # None / empty / non-array / non-float64 entries: the careful path, chunk by chunk
      parts = []
      counts[:] = 0
      for u, chunk in enumerate(chunks):
        if chunk is None or len(chunk) == 0:
          continue
        arr = np.ascontiguousarray(chunk, dtype=np.float32)
        if arr.ndim != 2 or arr.shape[1] != dim:
          raise ValueError('chunk does not match observation_dim')
        parts.append(arr)
        counts[u] = arr.shape[0]
      frames64 = np.concatenate(parts) if parts else np.zeros((0, dim), dtype=np.float32)
    if frames64.shape[0] and frames64.shape[1] != dim:
      raise ValueError('chunk does not match observation_dim')
    frames = frames64.astype(np.float32, copy=False)
    if bias is not None:
      self.set_frame_bias(bias)
    if speakers is not None:
      self.set_stream_speakers(speakers)
    rc = self._lib.uis_stream_push(self._handle, frames.ctypes.data_as(_fp) if len(frames) else None, self._stream_counts_ptr)
    self._check(rc, 'uis_stream_push')
    self._stream_have += counts

  def _producer(self, stream):
    """producer_stream of the tensor entry points: `stream` (a raw hipStream_t as an int, 0: the default stream), or,
    for None, the stream torch is issuing work to on this device at this moment."""
    if stream is None:
      import torch  # pylint: disable=import-outside-toplevel
      stream = torch.cuda.current_stream(self.device).cuda_stream
    return ctypes.c_void_p(int(stream) or None)

  def ingest_tensors(self, source, lengths=None, out=None, stream=None):
    """uis_ingest_tensors, the gather kernel alone: `source` as tensor_table takes it -> the packed float32
    [sum rows, D] device tensor (`out`: written from its first row, must be contiguous and hold that many)."""
    import torch  # pylint: disable=import-outside-toplevel
    table, keep = tensor_table(source, self.observation_dim, lengths, self.device, 'tensors')
    total = check_tensor_table(table, self.observation_dim, None if out is None else int(out.shape[0]))
    if out is None:
      out = torch.empty((total, self.observation_dim), dtype=torch.float32, device='cuda:{}'.format(self.device))
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.ndim != 2 or out.shape[1] != self.observation_dim:
      raise ValueError('out must be a contiguous float32 [rows, D] tensor')
    self._check(self._lib.uis_ingest_tensors(self._handle, _table_ptr(table), len(table), self._producer(stream),
                                             ctypes.c_void_p(out.data_ptr() or None), int(out.shape[0])),
                'uis_ingest_tensors', ok=(UIS_OK,))
    del keep
    return out[:total]

  def decode_tensors(self, source, beam_size, look_ahead, test_iteration, max_clusters=0, flags=0, want_beam_scores=False,
                     n_streams=0, level_cap=0, limits=None, bias=None, speakers=None, min_turn=None, lengths=None,
                     stream=None):
    """Decode utterances that live in device tensors (uis_tensors_decode): `source` and `lengths` as tensor_table
    takes them, everything else as decode_f64.

    Returns the dict of decode() with `labels` an int32 DEVICE tensor (packed in utterance order) and `scores` on the
    host (float32 [U]; `scores_device`: the tensor they came from), and `empty` (bool [U]): the utterances whose beam
    became empty -- their score is not finite, which no surviving hypothesis' is (every select drops such candidates)."""
    import torch  # pylint: disable=import-outside-toplevel
    table, keep = tensor_table(source, self.observation_dim, lengths, self.device)
    total = check_tensor_table(table, self.observation_dim)
    n_utt = len(table)
    offsets = _offsets(table['rows'])
    where = 'cuda:{}'.format(self.device)
    labels = torch.empty(max(total, 1), dtype=torch.int32, device=where)
    scores = torch.empty(max(n_utt, 1), dtype=torch.float32, device=where)
    opts = make_opts(beam_size, look_ahead, test_iteration, max_clusters, flags, n_streams, level_cap)
    producer = self._producer(stream)

    def call(handle, blocks, _, count, *rest):   # (_run_decode's argument order, with the table in the frames' place)
      return self._lib.uis_tensors_decode(handle, blocks, count, producer, *rest)

    out = self._run_decode(call, 'uis_tensors_decode', opts, _table_ptr(table), offsets, offsets,
                           ctypes.c_void_p(labels.data_ptr()), ctypes.c_void_p(scores.data_ptr()), limits, bias, speakers,
                           min_turn)
    del keep
    host_scores = scores[:n_utt].cpu().numpy()
    out.update(labels=labels[:total], scores=host_scores, scores_device=scores[:n_utt],
               empty=~np.isfinite(host_scores) & (table['rows'] > 0))
    return self._with_decode_info(out, n_utt, beam_size, want_beam_scores)

  def stream_push_tensors(self, chunks, bias=None, speakers=None, stream=None, table=None):
    """stream_push with the new frames in device tensors (uis_tensors_stream_push): a list with one [n_u, D] tensor
    (or None) per utterance, or ONE [n_utt, n, D] tensor; float64, float32, float16 or bfloat16, any row stride.  The
    frames never leave the device.  bias, speakers: as stream_push.  table: tensor_table's result for these chunks, where
    the caller has already made it."""
    if len(chunks) != self._stream_n:
      raise ValueError('one chunk (or None) per utterance')
    table, keep = table or tensor_table(chunks, self.observation_dim, None, self.device, 'chunks')
    if isinstance(chunks, (list, tuple)):   # (the table of one checked [U, n, D] tensor holds nothing a check could find)
      check_tensor_table(table, self.observation_dim)
    if bias is not None:
      self.set_frame_bias(bias)
    if speakers is not None:
      self.set_stream_speakers(speakers)
    rc = self._lib.uis_tensors_stream_push(self._handle, _table_ptr(table), self._producer(stream))
    self._check(rc, 'uis_tensors_stream_push')
    del keep
    self._stream_have += table['rows']

  def stream_received(self):
    """Frames per utterance the open session holds (pushed or primed, not yet committed): int64 [n_utt]."""
    return self._stream_have.copy()

  def stream_prime(self, chunks, labels, speakers=None):
    """Prime utterances of the open session with labeled prefixes (uis_stream_prime).

    chunks: one [P_u, D] array (or None / empty) per utterance; labels: one int sequence in first-appearance
    form (or None / empty) per utterance, P_u entries; speakers: the prefixes' tags, uint8 in the call's frame order
    (utterance-major), or None (set_stream_speakers).  Returns the float32 prefix scores [n_utt] (0 where
    nothing was primed).  A refusal (HipLibraryError with .status) leaves the session as it was."""
    if len(chunks) != self._stream_n or len(labels) != self._stream_n:
      raise ValueError('one chunk and one label sequence (or None) per utterance')
    dim = self.observation_dim
    parts, lab_parts = [], []
    counts = np.zeros(self._stream_n, dtype=np.int64)
    for u, (chunk, lab) in enumerate(zip(chunks, labels)):
      n = 0 if chunk is None else len(chunk)
      n_lab = 0 if lab is None else len(lab)
      if n != n_lab:
        raise ValueError('utterance {}: {} labels for a prefix of {} frames'.format(u, n_lab, n))
      if n == 0:
        continue
      arr = np.ascontiguousarray(chunk, dtype=np.float32)
      if arr.ndim != 2 or arr.shape[1] != dim:
        raise ValueError('chunk does not match observation_dim')
      parts.append(arr)
      lab_parts.append(np.asarray(lab, dtype=np.int32).reshape(-1))
      counts[u] = n
    frames = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, dim), dtype=np.float32)
    flat = np.ascontiguousarray(np.concatenate(lab_parts)) if lab_parts else np.zeros(0, dtype=np.int32)
    offsets = _offsets(counts)
    scores = np.zeros(self._stream_n, dtype=np.float32)
    if speakers is not None:
      self.set_stream_speakers(speakers)
    rc = self._lib.uis_stream_prime(
        self._handle, _ptr(frames) if len(frames) else None, _i64(offsets),
        _i32(flat) if len(flat) else None, _ptr(scores))
    self._check(rc, 'uis_stream_prime', ok=(UIS_OK,))
    self._stream_have += counts
    return scores

  def stream_commit(self, horizon=None):
    """Hand out the labels that are final and move the session's window behind them (uis_stream_commit).

    horizon: None (only the stable prefix is committed), or one int per utterance (negative: none for that
    utterance): frames older than the newest `horizon` are decided in favour of the best hypothesis, and the
    hypotheses that disagree with it there leave the beam.  Returns (labels, dropped): per utterance the int32
    labels committed by this call (an even number of them), and int32 [n_utt] hypotheses pruned.  Afterwards
    stream_received(), stream_labels() and stream_nbest() speak about the window: the frames not yet committed."""
    n_utt = self._stream_n
    hz_ptr = None
    if horizon is not None:
      hz = np.ascontiguousarray(horizon, dtype=np.int32).reshape(-1)
      if hz.shape[0] != n_utt:
        raise ValueError('one horizon per utterance')
      hz_ptr = _i32(hz)
    total = int(self._stream_have.sum())
    labels = np.empty(max(total, 1), dtype=np.int32)
    counts = np.zeros(n_utt, dtype=np.int32)
    dropped = np.zeros(n_utt, dtype=np.int32)
    rc = self._lib.uis_stream_commit(self._handle, hz_ptr, _i32(labels), total, _i32(counts), _i32(dropped))
    self._check(rc, 'uis_stream_commit', ok=(UIS_OK,))
    self._stream_have -= counts
    return _cut(labels, _offsets(counts)), dropped

  def stream_committed(self):
    """Frames per utterance committed so far (uis_stream_committed): int64 [n_utt]."""
    out = np.zeros(self._stream_n, dtype=np.int64)
    self._check(self._lib.uis_stream_committed(self._handle, _i64(out)), 'uis_stream_committed')
    return out

  def stream_restart(self, which):
    """End the utterances selected by `which` and leave their slots fresh (uis_stream_restart).

    which: one truth value per utterance.  Returns (labels, scores, overflow, status): per utterance the int32
    labels of its window at this moment (what stream_labels() would give; empty for an utterance not selected),
    float32 [n_utt] scores and int32 [n_utt] overflow words from before the reset (entries of utterances not
    selected: nan and 0), and UIS_OK or UIS_ERR_CLUSTER_CAP (a selected utterance had hit the cap; the restart has
    happened all the same).  A refusal (HipLibraryError with .status) leaves the session as it was."""
    n_utt = self._stream_n
    sel = np.ascontiguousarray([1 if w else 0 for w in which], dtype=np.int32)
    if sel.shape[0] != n_utt:
      raise ValueError('one selection flag per utterance')
    total = int(self._stream_have[sel != 0].sum())
    labels = np.empty(max(total, 1), dtype=np.int32)
    counts = np.zeros(n_utt, dtype=np.int32)
    scores = np.full(n_utt, np.nan, dtype=np.float32)
    overflow = np.zeros(n_utt, dtype=np.int32)
    rc = self._check(self._lib.uis_stream_restart(
        self._handle, _i32(sel), _i32(labels), total, _i32(counts), _ptr(scores), _i32(overflow)), 'uis_stream_restart')
    self._stream_have[sel != 0] = 0
    return _cut(labels, _offsets(counts)), scores, overflow, rc

  def stream_retire(self, which=None, clusters=None):
    """Delete clusters that no live hypothesis can still name (uis_stream_retire).

    clusters None: every retirable cluster of the utterances selected by `which` (one truth value per utterance;
    None: all of them); the others are only queried.  clusters given (then which must be None): one ascending
    sequence of cluster indices (or None / empty: a query) per utterance.  Returns dict(retired, K, retirable,
    max_clusters): per utterance the int32 indices retired, in the numbering before the call; int32 [n_utt] the
    largest K over the live hypotheses afterwards; per utterance the indices that were retirable before the call.
    A refusal (HipLibraryError with .status UIS_ERR_INVALID_ARG) leaves the session as it was."""
    n_utt = self._stream_n
    which_ptr = off_ptr = sel_ptr = None
    if clusters is not None:
      if which is not None:
        raise ValueError('which and clusters exclude each other')
      if len(clusters) != n_utt:
        raise ValueError('one sequence of cluster indices (or None) per utterance')
      parts = [np.zeros(0, dtype=np.int32) if c is None else np.asarray(c, dtype=np.int32).reshape(-1) for c in clusters]
      offsets = _offsets([len(x) for x in parts])
      flat = np.ascontiguousarray(np.concatenate(parts), dtype=np.int32)
      off_ptr = _i64(offsets)
      sel_ptr = _i32(flat) if len(flat) else None
    elif which is not None:
      sel = np.ascontiguousarray([1 if w else 0 for w in which], dtype=np.int32)
      if sel.shape[0] != n_utt:
        raise ValueError('one selection flag per utterance')
      which_ptr = _i32(sel)
    cap = self.stream_max_clusters()
    retired = np.zeros((n_utt, cap), dtype=np.int32)
    retirable = np.zeros((n_utt, cap), dtype=np.int32)
    counts = np.zeros(n_utt, dtype=np.int32)
    able = np.zeros(n_utt, dtype=np.int32)
    k_out = np.zeros(n_utt, dtype=np.int32)
    rc = self._lib.uis_stream_retire(
        self._handle, which_ptr, off_ptr, sel_ptr, _i32(retired), _i32(counts), _i32(k_out), _i32(retirable), _i32(able))
    self._check(rc, 'uis_stream_retire', ok=(UIS_OK,))
    return {'retired': [retired[u, :counts[u]].copy() for u in range(n_utt)], 'K': k_out,
            'retirable': [retirable[u, :able[u]].copy() for u in range(n_utt)], 'max_clusters': cap}

  def stream_export_bound(self, utt=0):
    """The capacity stream_export needs (uis_stream_export_bound): host only."""
    out = ctypes.c_int64(0)
    self._check(self._lib.uis_stream_export_bound(self._handle, int(utt), ctypes.byref(out)), 'uis_stream_export_bound')
    return int(out.value)

  def stream_export(self, utt):
    """One utterance of the open session as bytes (uis_stream_export): the library's blob, canonical -- a function
    of the utterance's state alone.  Changes nothing.  A refusal is a HipLibraryError with .status
    (UIS_ERR_CLUSTER_CAP: the utterance has hit the cluster cap; UIS_ERR_INVALID_ARG: its beam is empty)."""
    if self._export_buf is None or len(self._export_buf) < self.stream_export_bound(utt):
      self._export_buf = ctypes.create_string_buffer(self.stream_export_bound(utt))
    n = ctypes.c_int64(0)
    rc = self._lib.uis_stream_export(self._handle, int(utt), self._export_buf, len(self._export_buf), ctypes.byref(n))
    self._check(rc, 'uis_stream_export', ok=(UIS_OK,))
    return ctypes.string_at(self._export_buf, n.value)

  def stream_import(self, utt, blob):
    """Put an exported utterance into slot `utt` of the open session, which must have received nothing
    (uis_stream_import).  A refusal (HipLibraryError with .status) leaves the session as it was."""
    blob = bytes(blob)
    rc = self._lib.uis_stream_import(self._handle, int(utt), blob, len(blob))
    self._check(rc, 'uis_stream_import', ok=(UIS_OK,))
    self._stream_have[int(utt)] = blob_info(blob)['N']

  def stream_bindings(self):
    """uis_stream_bindings: int32 [n_utt, 128] -- column g (1 .. 127) the cluster the best hypothesis binds tag g to, in
    the numbering of stream_labels() at this moment, -1 = unbound; column 0 the number of bound tags."""
    out = np.full((self._stream_n, 128), -1, dtype=np.int32)
    self._check(self._lib.uis_stream_bindings(self._handle, _i32(out)), 'uis_stream_bindings', ok=(UIS_OK,))
    return out

  def stream_max_clusters(self):
    """max_clusters of the open session (what uis_stream_begin made of the option: 0 means 16)."""
    return self._stream_cap

  def stream_labels(self):
    """Best-hypothesis labels of everything received so far: (list of int32 arrays, scores, overflow, status)."""
    labels = np.empty(max(int(self._stream_have.sum()), 1), dtype=np.int32)
    scores = np.empty(self._stream_n, dtype=np.float32)
    overflow = np.zeros(self._stream_n, dtype=np.int32)
    rc = self._check(self._lib.uis_stream_labels(self._handle, _i32(labels), _ptr(scores), _i32(overflow)),
                     'uis_stream_labels')
    return _cut(labels, _offsets(self._stream_have)), scores, overflow, rc

  def stream_end(self):
    self._check(self._lib.uis_stream_end(self._handle), 'uis_stream_end')

  def _last_layout(self, who):
    """(offsets, beam_size) of the last decode, for `who` to size its buffers: the offsets this object remembers,
    checked against what the library says of its last decode (uis_last_decode_shape)."""
    offsets = self._last_offsets
    if offsets is None:
      offsets = np.zeros(1, dtype=np.int64)  # (no decode yet: the library refuses the readout itself)
    n_lib, beam = ctypes.c_int32(0), ctypes.c_int32(0)
    self._check(self._lib.uis_last_decode_shape(self._handle, ctypes.byref(n_lib), ctypes.byref(beam)),
                'uis_last_decode_shape')
    if int(n_lib.value) != offsets.shape[0] - 1:  # (a decode that did not go through this object's wrappers: its layout is not known here)
      raise HipLibraryError('{}: the library\'s last decode had {} utterances, this object remembers {}'.format(
          who, int(n_lib.value), offsets.shape[0] - 1))
    return offsets, int(beam.value)

  # ---- n-best readout (uis_last_decode_nbest / uis_stream_nbest)
  def _nbest(self, call, what, n_best, offsets, *more):
    """One n-best call of the library over utterances laid out by `offsets`; `more`: the call's further arguments.
    Returns (last_nbest's dict, status)."""
    n_best = int(n_best)
    n_utt = offsets.shape[0] - 1
    total = max(n_best, 0) * int(offsets[-1])
    labels = np.empty(max(total, 1), dtype=np.int32)
    scores = np.empty(max(n_utt * max(n_best, 0), 1), dtype=np.float32)
    counts = np.zeros(max(n_utt, 1), dtype=np.int32)
    rc = self._check(call(self._handle, n_best, _i32(labels), total, _ptr(scores), _i32(counts), *more), what)
    per_utt = [labels[n_best * int(a):n_best * int(b)].reshape(n_best, int(b - a)).copy()
               for a, b in zip(offsets[:-1], offsets[1:])]
    return {'labels': per_utt, 'scores': scores[:n_utt * n_best].reshape(n_utt, n_best), 'counts': counts[:n_utt]}, rc

  def last_nbest(self, n_best):
    """Every hypothesis of the last decode's final beam (uis_last_decode_nbest).

    Returns a dict: labels -- per utterance an int32 [n_best, N_u] array, row k = hypothesis k in the
    form of decode()'s labels, rows >= counts[u] filled with -1; scores float32 [U, n_best], ascending,
    +inf padded; counts int32 [U] = min(n_best, live hypotheses), 0 for an utterance that hit the
    cluster cap."""
    offsets, _ = self._last_layout('last_nbest')
    return self._nbest(self._lib.uis_last_decode_nbest, 'uis_last_decode_nbest', n_best, offsets)[0]

  def stream_nbest(self, n_best):
    """Every hypothesis of the open session's beam for everything received so far (uis_stream_nbest).

    The dict of last_nbest() plus stable (int64 [U]: leading frames whose labels are final) and status."""
    stable = np.zeros(self._stream_n, dtype=np.int64)
    out, rc = self._nbest(self._lib.uis_stream_nbest, 'uis_stream_nbest', n_best, _offsets(self._stream_have),
                          _i64(stable))
    out['stable'] = stable
    out['status'] = rc
    return out

  # ---- posterior readout (uis_last_decode_posterior / uis_stream_posterior)
  def _posterior(self, call, what, temperature, offsets, beam):
    n_utt = offsets.shape[0] - 1
    total = int(offsets[-1])
    conf = np.zeros(max(total, 1), dtype=np.float32)
    change = np.zeros(max(total, 1), dtype=np.float32)
    weights = np.zeros(max(n_utt * beam, 1), dtype=np.float32)
    counts = np.zeros(max(n_utt, 1), dtype=np.int32)
    rc = self._check(call(self._handle, float(temperature), _ptr(conf), _ptr(change), total, _ptr(weights),
                          _i32(counts)), what)
    return {'confidence': _cut(conf, offsets), 'change': _cut(change, offsets),
            'weights': weights[:n_utt * beam].reshape(n_utt, beam), 'counts': counts[:n_utt], 'status': rc}

  def last_posterior(self, temperature=1.0):
    """Per-frame confidence of the last decode's labels from its final beam (uis_last_decode_posterior).

    With w_k = softmax(-scores / temperature) over the live hypotheses, returns a dict: confidence -- per
    utterance a float32 [N_u] array, the weight of the hypotheses that agree with the best one's label at that
    frame; change -- likewise, the weight of the hypotheses with a speaker turn between frames t - 1 and t
    (change[0] = 0); weights float32 [U, beam_size], rank order, 0 past the live ones; counts int32 [U], the live
    hypotheses (0 for an utterance that hit the cluster cap: zeros everywhere); status."""
    offsets, beam = self._last_layout('last_posterior')
    return self._posterior(self._lib.uis_last_decode_posterior, 'uis_last_decode_posterior', temperature, offsets, beam)

  def stream_posterior(self, temperature=1.0):
    """The same for the open session's window: everything received and not yet committed (uis_stream_posterior).
    A window that a commit emptied has counts 1, weights[u, 0] = 1 and no frames."""
    return self._posterior(self._lib.uis_stream_posterior, 'uis_stream_posterior', temperature,
                           _offsets(self._stream_have), self._stream_beam)

  def decode_host(self, frames_ptr, offsets, beam_size, look_ahead, test_iteration,
                  labels_ptr, scores_ptr, max_clusters=0, flags=0, limits=None, bias=None, speakers=None,
                  min_turn=None):
    """uis_decode on raw HOST pointers (e.g. pinned buffers from uis_host_alloc or torch)."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    opts = make_opts(beam_size, look_ahead, test_iteration, max_clusters, flags, 0)
    return self._run_decode(
        self._lib.uis_decode, 'uis_decode', opts, ctypes.cast(ctypes.c_void_p(int(frames_ptr)), _fp), offsets,
        offsets.copy(), ctypes.cast(ctypes.c_void_p(int(labels_ptr)), _i32p),
        ctypes.cast(ctypes.c_void_p(int(scores_ptr)), _fp) if scores_ptr else None, limits, bias, speakers, min_turn)

  # ---- evaluation on the device (uis_eval_*)
  @staticmethod
  def _eval_args(offsets):
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n_utt = offsets.shape[0] - 1
    matched = np.zeros(max(n_utt, 1), dtype=np.int64)
    return offsets, n_utt, matched

  def eval_matched(self, labels_a, labels_b, offsets):
    """Matched positions per utterance under the best label mapping (host int32 arrays in)."""
    labels_a = np.ascontiguousarray(labels_a, dtype=np.int32)
    labels_b = np.ascontiguousarray(labels_b, dtype=np.int32)
    offsets, n_utt, matched = self._eval_args(offsets)
    if labels_a.shape != labels_b.shape or labels_a.shape[0] != int(offsets[-1]):
      raise ValueError('both label arrays must hold offsets[-1] entries')
    self._check(self._lib.uis_eval_accuracy(
        self._handle, _i32(labels_a), _i32(labels_b), _i64(offsets), n_utt, _i64(matched)), 'uis_eval_accuracy')
    return matched[:n_utt]

  def eval_matched_device(self, d_labels_a_ptr, d_labels_b_ptr, offsets):
    """Same with both label sequences resident in HBM (raw device pointers)."""
    offsets, n_utt, matched = self._eval_args(offsets)
    self._check(self._lib.uis_eval_accuracy_device(
        self._handle, ctypes.c_void_p(int(d_labels_a_ptr)), ctypes.c_void_p(int(d_labels_b_ptr)),
        _i64(offsets), n_utt, _i64(matched)), 'uis_eval_accuracy_device')
    return matched[:n_utt]

  def eval_last_decode(self, truth, n_utt):
    """Matched positions of the last decode()'s labels (still in HBM) against `truth`."""
    truth = np.ascontiguousarray(truth, dtype=np.int32)
    matched = np.zeros(max(int(n_utt), 1), dtype=np.int64)
    self._check(self._lib.uis_eval_last_decode(self._handle, _i32(truth), int(n_utt), _i64(matched)),
                'uis_eval_last_decode')
    return matched[:int(n_utt)]

  def decode_device(self, d_frames_ptr, offsets, beam_size, look_ahead,
                    test_iteration, d_labels_ptr, d_scores_ptr, max_clusters=0,
                    flags=0, n_streams=0, limits=None, bias=None, speakers=None, min_turn=None):
    """Decode with frames/labels/scores already resident in HBM (raw pointers)."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    opts = make_opts(beam_size, look_ahead, test_iteration, max_clusters, flags, n_streams)
    return self._run_decode(
        self._lib.uis_decode_device, 'uis_decode_device', opts, ctypes.c_void_p(int(d_frames_ptr)), offsets,
        offsets.copy(), ctypes.c_void_p(int(d_labels_ptr)),
        ctypes.c_void_p(int(d_scores_ptr) if d_scores_ptr else None), limits, bias, speakers, min_turn)


def flatten_params(params):
  """The trainer's flat parameter vector (include/uisrnn_hip.h) from a parameter dict."""
  parts = []
  for l in range(int(params['rnn_depth'])):
    for key in ('gru_weight_ih', 'gru_weight_hh', 'gru_bias_ih', 'gru_bias_hh'):
      parts.append(_f32(params[key][l]).ravel())
  for key in ('linear_mean1_weight', 'linear_mean1_bias', 'linear_mean2_weight',
              'linear_mean2_bias', 'rnn_init_hidden', 'sigma2'):
    parts.append(_f32(params[key]).ravel())
  return np.concatenate(parts)


def unflatten_params(flat, like):
  """A parameter dict shaped like `like` (uisrnn_amd.weights) holding the values of `flat`."""
  out = dict(like)
  pos = 0

  def take(shape):
    nonlocal pos
    n = int(np.prod(shape))
    a = np.array(flat[pos:pos + n], dtype=np.float32).reshape(shape)
    pos += n
    return a

  for key in ('gru_weight_ih', 'gru_weight_hh', 'gru_bias_ih', 'gru_bias_hh'):
    out[key] = list(like[key])
  for l in range(int(like['rnn_depth'])):
    for key in ('gru_weight_ih', 'gru_weight_hh', 'gru_bias_ih', 'gru_bias_hh'):
      out[key][l] = take(np.shape(like[key][l]))
  for key in ('linear_mean1_weight', 'linear_mean1_bias', 'linear_mean2_weight',
              'linear_mean2_bias', 'rnn_init_hidden', 'sigma2'):
    out[key] = take(np.shape(like[key]))
  assert pos == len(flat), (pos, len(flat))
  return out


class Trainer:
  """Owns one uis_trainer: the weights being trained, their Adam state and the training data."""

  def __init__(self, params, device=0, learning_rate=1e-3, regularization_weight=1e-5,
               grad_max_norm=5.0, sigma_alpha=1.0, sigma_beta=1.0, estimate_sigma2=True,
               dropout=0.0, dropout_key=0):
    self._lib = load_library()
    self._handle = None
    self.params_like = params
    self.observation_dim = int(params['observation_dim'])
    p = dict(params)
    if p.get('transition_bias') is None:
      p['transition_bias'] = 0.0   # not used by the trainer
    desc, keep = make_desc(p)
    opts = TrainOpts()
    opts.learning_rate = float(learning_rate)
    opts.regularization_weight = float(regularization_weight)
    opts.grad_max_norm = float(grad_max_norm)
    opts.sigma_alpha = float(sigma_alpha)
    opts.sigma_beta = float(sigma_beta)
    opts.dropout = float(dropout)
    opts.dropout_key = int(dropout_key) & 0xffffffffffffffff
    opts.estimate_sigma2 = 1 if estimate_sigma2 else 0
    handle = ctypes.c_void_p()
    rc = self._lib.uis_train_create(ctypes.byref(desc), ctypes.byref(opts), int(device),
                                    ctypes.byref(handle))
    del keep
    if rc != UIS_OK:
      raise HipLibraryError('uis_train_create failed ({}): {}'.format(rc, last_error(self._lib)))
    self._handle = handle
    count = ctypes.c_int64()
    self._check(self._lib.uis_train_param_count(self._handle, ctypes.byref(count)),
                'uis_train_param_count')
    self.n_params = count.value
    self._lengths = None

  def _check(self, rc, what):
    if rc != UIS_OK:
      _raise_status(self._lib, rc, what)

  def close(self):
    if getattr(self, '_handle', None):
      self._lib.uis_train_destroy(self._handle)
      self._handle = None

  def __del__(self):
    try:
      self.close()
    except Exception:  # pylint: disable=broad-except
      pass

  def set_data(self, sub_sequences):
    """Upload the training sub-sequences (a list of [rows, D] arrays) once."""
    rows = [len(s) for s in sub_sequences]
    offsets = np.zeros(len(rows) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(rows)
    pool = _f32(np.concatenate([np.asarray(s).reshape(-1, self.observation_dim)
                                for s in sub_sequences], axis=0))
    self._check(self._lib.uis_train_set_data(self._handle, _ptr(pool), _i64(offsets), len(rows)), 'uis_train_set_data')
    self._lengths = np.asarray(rows)

  def step(self, batch_idx, want_losses=True):
    """One iteration on the sub-sequences batch_idx (longest first): (loss, loss1, loss2, loss3)."""
    idx = np.ascontiguousarray(batch_idx, dtype=np.int32)
    out = np.zeros(4, dtype=np.float32)
    self._check(self._lib.uis_train_step(self._handle, _i32(idx), len(idx), _ptr(out) if want_losses else None),
                'uis_train_step')
    return tuple(float(v) for v in out) if want_losses else None

  def flat_params(self):
    out = np.empty(self.n_params, dtype=np.float32)
    self._check(self._lib.uis_train_get_params(self._handle, _ptr(out), self.n_params),
                'uis_train_get_params')
    return out

  def flat_grads(self):
    out = np.empty(self.n_params, dtype=np.float32)
    self._check(self._lib.uis_train_get_grads(self._handle, _ptr(out), self.n_params),
                'uis_train_get_grads')
    return out

  def params(self):
    """The current weights as a parameter dict (the rest of the dict as given at creation)."""
    return unflatten_params(self.flat_params(), self.params_like)

  def grads(self):
    """The last iteration's gradients (after clipping), shaped like the parameters."""
    return unflatten_params(self.flat_grads(), self.params_like)
