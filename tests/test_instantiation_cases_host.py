"""The case table of tests/test_gpu_instantiations.py (tests/instantiation_cases.py) held to its own rules on the CPU,
with the oracle alone, so that the matrix cannot degrade quietly: a case whose reference leaves its kernel's limits would
fall back on the device and prove nothing; a table row without a case would go untested.

The utterance counts depend on the device's XCD count; a whole MI355X (8) is what is checked here.
"""

import ctypes
import functools

import numpy as np
import pytest

import instantiation_cases as ic
from uisrnn_amd import _capi

NCL = 8

_ALL = [case for row in ic.ROWS for case in ic.CASES[row]]


def test_the_case_table_is_the_librarys_kernel_table():
  """Every entry of the seven kernel tables, as the library enumerates them (uis_decode_kernel_table: no device
  needed), has its cases, and no case names an entry that is not there."""
  table = _capi.decode_kernel_table()
  assert len(table) == len(set(table)), 'an instantiation is listed twice'
  assert len(ic.ROWS) == len(set(ic.ROWS))
  assert set(ic.CASES) == set(ic.ROWS) == set(table), sorted(set(table) ^ set(ic.ROWS))
  for row in ic.ROWS:
    assert ic.CASES[row], row
  assert len({ic.row_id(row) for row in ic.ROWS}) == len(ic.ROWS)
  # the capacity argument is honoured: a short buffer is not overrun, and the count is still the whole table's
  lib = _capi.load_library()
  rows = np.full((3, 5), -1, dtype=np.int32)
  assert lib.uis_decode_kernel_table(rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 2) == len(table)
  assert (rows[:2, 0] > 0).all() and (rows[2] == -1).all()
  # ... and the per-handle entry refuses a null handle instead of reading through it
  out = (ctypes.c_int32 * 5)()
  assert lib.uis_last_decode_instantiation(None, out) == _capi.UIS_ERR_INVALID_ARG


def dim_is_exact(case):
  """What plan_decode calls exact: no padded feature, every hidden unit's mask open (the embedded sizes 257 .. 384)."""
  return case.dim == case.row[2] and (case.hidden == case.row[1] or 257 <= case.hidden <= 384)


@functools.lru_cache(maxsize=None)
def reference(name):
  from oracle import oracle
  oracle.lib()
  case = {c.name: c for c in _ALL}[name]
  return oracle.decode(case.params(), case.utterances(NCL), case.beam, case.look_ahead, case.test_iteration, n_threads=8)


@pytest.mark.parametrize('case', _ALL, ids=[c.name for c in _ALL])
def test_case_stays_inside_its_kernels_limits(case):
  family, hp, dp, variant, persist = case.row
  ref = reference(case.name)
  lens = case.lens(NCL)
  steps = case.test_iteration * max(lens)
  # the cap: what the oracle's survivors hold (and an intermediate look-ahead level up to look_ahead - 1 more), the
  # select of the row's kernel
  assert int(ref['max_clusters'].max()) + case.look_ahead - 1 <= case.cap
  if case.look_ahead == 1:
    assert ic.select_fast_ok(case.beam, case.cap)
  if family in (ic.RS, ic.BIG_WS):
    assert ic.rs_select_ok(case.beam, case.cap, steps)
  # the search did something: a full final beam, a hypothesis of three clusters
  assert np.isfinite(ref['beam_scores']).all(axis=1).any()
  assert int(ref['max_clusters'].max()) >= 3
  for u, labels in enumerate(ref['labels']):
    assert (labels >= 0).all(), u
  # the utterances: ragged, one frame, a long one where the row allows it, uneven XCDs
  assert 1 in lens and len(set(lens)) > 1
  n_utt = len(lens)
  assert n_utt % NCL != 0
  many = family in (ic.BIG, ic.BIG_WS)
  if many:
    assert max(lens) <= 7 and case.test_iteration == 1 and sum(lens) <= 1500
  elif not (family == ic.WINDOW and variant == ic.CLS_C2):
    assert steps >= 2 * 16 + 1
  # reaching the row (plan_decode's thresholds)
  per_xcd = -(-n_utt // NCL)
  if family == ic.RS:
    assert per_xcd <= 8 and not case.flags
  elif family == ic.RESIDENT:
    assert n_utt <= 32 * NCL and (persist or case.flags & _capi.UIS_FLAG_OWNER_SELECT)
  elif family == ic.BIG_WS:
    assert n_utt == 20 * NCL + 1 and not case.flags
  elif family == ic.BIG:
    assert n_utt == 32 * NCL + 1 and bool(case.flags & _capi.UIS_FLAG_OWNER_SELECT) == (dp <= 256)
  elif family == ic.WINDOW:
    assert case.look_ahead == 2 and n_utt in (2, 3)
  elif family == ic.DEEP:
    assert case.depth == 2 and case.look_ahead == (2 if variant else 1)
  if persist:
    assert case.flags & _capi.UIS_FLAG_PERSISTENT and case.test_iteration == 1
    pushes = case.pushes(NCL)
    assert len(pushes) >= 2 and len({tuple(p) for p in pushes}) > 1 and max(max(p) for p in pushes) <= 16
    assert [sum(p[u] for p in pushes) for u in range(n_utt)] == lens
  # the shape classes' own beam / cap
  cls = variant if family not in (ic.RS, ic.DEEP) else (ic.CLS_C1 if family == ic.RS and variant == ic.RS_C1 else 0)
  want = {ic.CLS_C1: (10, 16), ic.CLS_C4: (20, 11), ic.CLS_C2: (50, 12)}
  if cls:
    assert (case.beam, case.cap) == want[cls] and dim_is_exact(case)
  else:
    assert (case.beam, case.cap) not in want.values()
  # the model pads to the row
  params = case.params()
  dim, hidden = int(params['observation_dim']), int(params['rnn_hidden_size'])
  assert (dim, hidden, int(params['rnn_depth'])) == (case.dim, case.hidden, case.depth)
  assert ic.padded_dims(dim, hidden) == (dp, hp)
  if case.model == 'exact':
    assert (dim, hidden) == (dp, hp)
  else:
    assert hidden < hp and (dim == dp if persist or cls else dim < dp)
    # barely: one unit / one feature fewer would pad to a smaller entry (385: the first size of four-block segments;
    # below it the three-block sizes share the 512 entry, and 257 is the first of those)
    assert hidden == {'padded': {128: 65, 256: 129, 512: 385}[hp], 'seg3': 257}[case.model]
    if hidden != 385:
      assert ic.padded_dims(dim, hidden - 1) != (dp, hp)
    if not persist and not cls:
      assert dim == 17 or ic.padded_dims(dim - 1, hidden) != (dp, hp)


def test_padding_rule_restated():
  """padded_dims at its edges: the segment length q = ceil(blocks / 8) decides."""
  assert ic.padded_dims(16, 64) is None and ic.padded_dims(16, 65) == (128, 128)
  assert ic.padded_dims(128, 128) == (128, 128) and ic.padded_dims(129, 129) == (256, 256)
  assert ic.padded_dims(256, 256) == (256, 256) and ic.padded_dims(257, 257) is None   # (dim 257 .. 384: q = 3)
  assert ic.padded_dims(256, 257) == (256, 512) and ic.padded_dims(256, 384) == (256, 512)
  assert ic.padded_dims(385, 385) == (512, 512) and ic.padded_dims(512, 512) == (512, 512)
  assert ic.padded_dims(513, 512) is None and ic.padded_dims(512, 513) is None
