"""Stream export / import's CPU side: the symbols, the refusals that need no device, the Python layer's trailer and
bookkeeping (OnlineSession.export_state / import_state / snapshot / restore, StreamPool.export / adopt) against a
stand-in decoder, and the blob validator of csrc/uis_blob.h under the host compiler's sanitizers.  No GPU needed.
"""

import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import golden_util
import test_restart_host as rh
import uisrnn_amd
from uisrnn_amd import _capi
from uisrnn_amd import build as lib_build
from uisrnn_amd import uisrnn as host

ROOT = os.path.normpath(os.path.join(os.path.dirname(golden_util.GOLDEN_DIR), '..'))
NAMES = ('uis_stream_export_bound', 'uis_stream_export', 'uis_stream_import')


def test_the_symbols_are_declared_bound_and_exported():
  header = open(os.path.join(ROOT, 'include', 'uisrnn_hip.h')).read()
  assert 'int32_t uis_stream_export_bound(uis_handle* h, int32_t utt, int64_t* bytes_out);' in header
  assert 'int32_t uis_stream_export(uis_handle* h, int32_t utt, void* blob, int64_t capacity, int64_t* bytes_out);' in header
  assert 'int32_t uis_stream_import(uis_handle* h, int32_t utt, const void* blob, int64_t bytes);' in header
  assert '#define UIS_ABI_VERSION 6' in header and _capi.UIS_ABI_VERSION == 6
  lib = lib_build.OUTPUT
  if not os.path.exists(lib):
    lib = lib_build.build()
  symbols = subprocess.run(['nm', '-D', '--defined-only', lib], check=True, capture_output=True, text=True).stdout
  exported = {line.split()[-1] for line in symbols.splitlines() if line.strip()}
  loaded = _capi.load_library()
  for name in NAMES:
    assert name in _capi.EXPORTED_SYMBOLS and name in exported and getattr(loaded, name).argtypes
  assert loaded.uis_abi_version() == 6
  for name in ('stream_export_bound', 'stream_export', 'stream_import'):
    assert hasattr(_capi.Decoder, name)
  for name in ('export_state', 'import_state', 'snapshot', 'restore'):
    assert hasattr(host.OnlineSession, name)
  assert hasattr(host.StreamPool, 'export') and hasattr(host.StreamPool, 'adopt')
  for source in ('uis_migrate.hip', 'uis_blob.h'):
    assert any(d.endswith(os.path.join('csrc', source)) for d in lib_build.DEPENDS)


def test_without_a_handle_the_calls_refuse_and_write_nothing():
  lib = _capi.load_library()
  n = ctypes.c_int64(-7)
  buf = ctypes.create_string_buffer(b'\x55' * 64, 64)
  assert lib.uis_stream_export_bound(None, 0, ctypes.byref(n)) == _capi.UIS_ERR_INVALID_ARG
  assert 'null handle' in _capi.last_error(lib)
  assert lib.uis_stream_export(None, 0, buf, 64, ctypes.byref(n)) == _capi.UIS_ERR_INVALID_ARG
  assert 'null handle' in _capi.last_error(lib)
  assert lib.uis_stream_import(None, 0, buf, 64) == _capi.UIS_ERR_INVALID_ARG
  assert 'null handle' in _capi.last_error(lib)
  assert n.value == -7 and buf.raw == b'\x55' * 64


# ---- the Python trailer

def _core(n_window, committed, ks=(0,), beam=2):
  """Bytes with the head of a library blob (what _capi.blob_info reads) and nothing else of one."""
  total = _capi._BLOB_HEAD.size + 16 * len(ks) + 16   # pylint: disable=protected-access
  head = _capi._BLOB_HEAD.pack(_capi.BLOB_MAGIC, 1, 3, 1, beam, 4, 16, 8, 16, 1, 0, 0, 0xfeed, total,   # pylint: disable=protected-access
                               committed, n_window, len(ks), sum(ks), sum(ks), 0.0, 0)
  return head + b''.join(struct.pack('<3if', k, k - 1, k, 0.0) for k in ks) + b'\0' * 16


def test_blob_info_reads_the_head():
  info = _capi.blob_info(_core(5, 40, ks=(2, 7, 3), beam=4))
  assert info == {'B': 4, 'bytes': 64 + 32 + 48 + 16, 'committed': 40, 'N': 5, 'live': 3, 'slots': 12, 'K': 7}
  with pytest.raises(ValueError, match='too short'):
    _capi.blob_info(b'UISB')
  with pytest.raises(ValueError, match='bad magic'):
    _capi.blob_info(b'\0' * 200)


def test_the_python_trailer_round_trips():
  core = _core(3, 6, ks=(4,))
  final, gone = [0, 1, 1, 4, 4, 5], [2, 3]
  blob = core + host._pack_state_trailer(core, final, gone)   # pylint: disable=protected-access
  assert host._unpack_state(blob) == (core, final, gone)      # pylint: disable=protected-access
  assert host._unpack_state(bytearray(blob)) == (core, final, gone)   # pylint: disable=protected-access
  empty = _core(0, 0)
  assert host._unpack_state(empty + host._pack_state_trailer(empty, [], [])) == (empty, [], [])   # pylint: disable=protected-access
  # the same state gives the same bytes
  assert blob == core + host._pack_state_trailer(core, list(final), tuple(gone))   # pylint: disable=protected-access
  # anything else is a ValueError: cut short, a flipped byte of the trailer, a trailer of another blob, no trailer
  for bad in (blob[:-1], blob + b'\0', core, blob[:len(core) + 5], b'', None, 17):
    with pytest.raises(ValueError, match='not an exported utterance state'):
      host._unpack_state(bad)   # pylint: disable=protected-access
  for at in range(len(core), len(blob)):
    damaged = bytearray(blob)
    damaged[at] ^= 0x40
    with pytest.raises(ValueError, match='not an exported utterance state'):
      host._unpack_state(bytes(damaged))   # pylint: disable=protected-access
  other = _core(3, 8, ks=(4,))
  with pytest.raises(ValueError, match='does not belong'):       # (six labels for eight committed frames)
    host._unpack_state(other + host._pack_state_trailer(core, final, gone))   # pylint: disable=protected-access


# ---- the bookkeeping, against a stand-in decoder

def _refusal(status, text):
  err = _capi.HipLibraryError(text)
  err.status = status
  return err


class _Movable(rh._StandIn):   # pylint: disable=protected-access
  """test_restart_host's stand-in (labels = positions in the stream) that can hand an utterance over: the blob is a
  head with the window's and the committed frame counts and K = k[u]."""

  def __init__(self, n_utt):
    super().__init__(n_utt)
    self.k = [0] * n_utt
    self.imports = []

  def stream_export(self, u):
    if u in self.dead:
      raise _refusal(_capi.UIS_ERR_CLUSTER_CAP, 'cluster cap')
    if u in self.empty_beam:
      raise _refusal(_capi.UIS_ERR_INVALID_ARG, 'the beam is empty')
    return _core(int(self.have[u]), int(self.done[u]), ks=(self.k[u],))

  def stream_import(self, u, blob):
    info = _capi.blob_info(blob)
    if self.have[u] + self.done[u]:
      raise _refusal(_capi.UIS_ERR_INVALID_ARG, 'has already received')
    self.imports.append(u)
    self.have[u], self.done[u], self.k[u] = info['N'], info['committed'], info['K']

  def stream_retire(self, which=None, clusters=None):
    n = len(self.have)
    retired = [np.asarray(c if c is not None else [], dtype=np.int32) for c in (clusters or [None] * n)]
    return {'retired': retired, 'K': np.array(self.k, dtype=np.int32), 'retirable': [np.zeros(0, dtype=np.int32)] * n, 'max_clusters': 16}


def _session(n_utt, max_frames=100, policy=False):
  session = rh._session(n_utt, max_frames)   # pylint: disable=protected-access
  session._decoder = _Movable(n_utt)
  if policy:
    session._bound, session._seen = [0] * n_utt, [{} for _ in range(n_utt)]
    session._set_retire_policy(12, 6, 16)
  return session


def test_a_moved_stream_keeps_its_labels_and_ids():
  src, dst = _session(3), _session(2, policy=True)
  src.push([np.zeros((9, 4)), np.zeros((4, 4)), None])
  assert src.commit([3, None, None])[0] == [0, 1, 2, 3, 4, 5]
  src.retire(clusters=[[1, 2], None, None])                      # ids 1 and 2 are gone: present index 1 is id 3
  src._decoder.k[0] = 5
  want = src.labels()[0]
  assert want == [0, 1, 2, 3, 4, 5, 8, 9, 10] and src._gone[0] == [1, 2]   # (committed labels keep their ids)
  blob = src.export_state(0)
  assert src.labels()[0] == want and src._decoder.have.tolist() == [3, 4, 0]     # export changes nothing
  assert src.export_state(np.int64(0)) == blob
  dst.import_state(1, blob)
  assert dst.labels() == [[], want] and dst.committed == [0, 6] and dst._gone == [[], [1, 2]]
  assert dst._bound[1] == 5 and dst._seen[1] == {c: c for c in range(6)}   # the policy: as after a query
  with pytest.raises(ValueError, match='already retired'):
    dst.retire(clusters=[None, [2]])                              # a retired id is never reused
  dst.push([None, np.zeros((2, 4))])
  assert dst.labels()[1] == want + [11, 12]
  assert dst.restart([1])[1] == (want + [11, 12], 11.0)           # restart returns the whole stream
  assert dst._final[1] == [] and dst._gone[1] == [] and dst._bound[1] == 0
  # a session that never retired takes it over all the same, and a blob without retired ids clears nothing it should keep
  plain = _session(1)
  plain.import_state(0, blob)
  assert plain._gone == [[1, 2]] and plain.labels() == [want]
  fresh = src.export_state(2)
  dst.import_state(1, fresh)
  assert dst.labels()[1] == [] and dst._gone[1] == []


def test_the_refusals_touch_nothing():
  session = _session(2)
  session.push([np.zeros((5, 4)), np.zeros((2, 4))])
  blob = session.export_state(0)
  for bad in (2, -1, True, 0.0, '0', None):
    with pytest.raises(ValueError, match='not in'):
      session.export_state(bad)
    with pytest.raises(ValueError, match='not in'):
      session.import_state(bad, blob)
  with pytest.raises(ValueError, match='not an exported utterance state'):
    session.import_state(1, blob[:-3])
  with pytest.raises(_capi.HipLibraryError) as err:               # the library's refusal: the slot has received frames
    session.import_state(1, blob)
  assert err.value.status == _capi.UIS_ERR_INVALID_ARG
  assert session._decoder.imports == [] and session.labels() == [list(range(5)), [0, 1]] and session._final == [[], []]
  session._decoder.dead.add(0)
  with pytest.raises(_capi.HipLibraryError) as err:
    session.export_state(0)
  assert err.value.status == _capi.UIS_ERR_CLUSTER_CAP


def test_snapshot_and_restore_skip_what_cannot_be_exported():
  session = _session(4)
  session.push([np.zeros((5, 4)), np.zeros((2, 4)), np.zeros((3, 4)), None])
  session.commit([1, None, None, None])
  session._decoder.dead.add(1)
  session._decoder.empty_beam.add(2)
  shots = session.snapshot()
  assert [s is None for s in shots] == [False, True, True, False]
  copy = _session(4)
  copy.restore(shots)
  assert copy._decoder.imports == [0, 3]
  assert copy.labels() == [list(range(5)), [], [], []] and copy.committed == [4, 0, 0, 0]
  class _Broken(_Movable):
    def stream_export(self, u):
      raise _refusal(_capi.UIS_ERR_HIP, 'a HIP call failed')
  session._decoder.__class__ = _Broken
  with pytest.raises(_capi.HipLibraryError):                       # anything but the two refusals is an error
    session.snapshot()
  for bad in (shots[:3], shots + [None], None, b''):
    with pytest.raises(ValueError, match='per utterance'):
      copy.restore(bad)


def test_stream_pool_export_and_adopt():
  a, b = host.StreamPool(_session(2)), host.StreamPool(_session(2))
  a.open('x')
  a.push({'x': np.zeros((3, 4))})
  blob = a.export('x')
  assert a.labels('x') == [0, 1, 2]                                # the key stays open
  with pytest.raises(KeyError):
    a.export('nobody')
  assert b.adopt('x', blob) == 0 and b.labels('x') == [0, 1, 2]
  with pytest.raises(KeyError):
    b.adopt('x', blob)                                             # the key is taken
  with pytest.raises(ValueError, match='not an exported utterance state'):
    b.adopt('y', blob[:10])
  assert b.open('y') == 1                                          # ... and the refused blob cost no slot
  with pytest.raises(RuntimeError, match='no free slot'):
    b.adopt('z', blob)                                             # a full pool
  assert b.finish('x') == ([0, 1, 2], 3.0)
  assert b.adopt('z', blob) == 0 and b.labels('z') == [0, 1, 2]


# ---- the validator under the host compiler's sanitizers

def test_the_blob_validator_refuses_every_damaged_blob(tmp_path):
  cxx = shutil.which(os.environ.get('CXX', '') or 'g++') or shutil.which('c++') or shutil.which('clang++')
  if not cxx:
    pytest.skip('no host C++ compiler')
  exe = str(tmp_path / 'blob_check')
  base = ['-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
  probe = str(tmp_path / 'probe.cpp')
  with open(probe, 'w') as f:
    f.write('int main() { return 0; }\n')
  # the runtime inside the program where the compiler offers that (the program then starts whatever else the
  # environment loads into it), else the compiler's default
  for flags in (base + ['-static-libasan', '-static-libubsan'], base + ['-static-libsan'], base):
    if subprocess.run([cxx] + flags + [probe, '-o', exe + '_probe'], capture_output=True).returncode == 0:
      break
  else:
    pytest.skip('the host compiler cannot link the sanitizer runtime')
  if subprocess.run([exe + '_probe'], capture_output=True).returncode != 0:
    pytest.skip('a program with the sanitizer runtime does not start in this environment')
  subprocess.run([cxx] + flags + ['-I', os.path.join(ROOT, 'uisrnn_amd', 'csrc'), os.path.join(ROOT, 'tests', 'blob_check_main.cpp'),
                                  '-o', exe], check=True)
  done = subprocess.run([exe], capture_output=True, text=True)
  assert done.returncode == 0 and done.stdout.startswith('blob_check: ok'), (done.returncode, done.stdout, done.stderr)
