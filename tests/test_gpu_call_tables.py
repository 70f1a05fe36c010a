"""Which entry point takes, refuses or leaves which per-call table (csrc/uis_call_tables.h), from
outside: the host program of tests/test_call_tables_host.py checks the rules, this checks that every entry point was
given the right one.

tiny_d16, 2 utterances of 3 frames, beam 2, window 8.  For every entry point and every table:
  1. the table is set with a length (7) that fits no call made here;
  2. the entry point is called with otherwise valid arguments.  A rule that LEAVEs the table lets the call succeed, one
     that TAKEs it makes the call report "<setter> gave 7 ..." (UIS_ERR_INVALID_ARG), one that REFUSEs it
     "<entry point> takes no ..." (UIS_ERR_UNSUPPORTED);
  3. whether the table is still pending: one of its consumers is called with a count that does not match; "<setter> gave
     7 ..." UIS_ERR_INVALID_ARG means it was pending, anything else that it was gone.  (uis_frame_speakers' table has
     no consumer while a session is open: there a call that refuses it is asked instead, uis_stream_committed.)
     A table is pending afterwards iff the rule is LEAVE;
  4. every table is cleared and the session ended.
RULES below is the table of DESIGN.md section 28, written out.
"""

import ctypes

import numpy as np
import pytest

import golden_util
from uisrnn_amd import _capi

pytestmark = pytest.mark.gpu

LEAVE, TAKE, REFUSE = 'leave', 'take', 'refuse'
TABLES = ('limits', 'bias', 'hint', 'stream_tags')
SETTER = {'limits': 'uis_decode_limits', 'bias': 'uis_frame_bias', 'hint': 'uis_frame_speakers', 'stream_tags': 'uis_stream_speakers'}
WRONG = 7   # (no call below has 7 utterances or 7 frames)
N_UTT, N_FRAMES, BEAM, WINDOW = 2, 3, 2, 8

_DECODE = (TAKE, TAKE, TAKE, LEAVE)
_SCORE = (LEAVE, TAKE, REFUSE, LEAVE)
_OTHER = (LEAVE, LEAVE, REFUSE, LEAVE)
_NONE = (LEAVE, LEAVE, LEAVE, LEAVE)
# entry point: (limits, bias, hint, stream_tags)
RULES = {
    'uis_decode': _DECODE, 'uis_decode_f64': _DECODE, 'uis_decode_device': _DECODE,
    'uis_score_labels': _SCORE, 'uis_score_speakers': _SCORE,
    'uis_stream_begin': (TAKE, LEAVE, REFUSE, LEAVE),
    'uis_stream_push': (LEAVE, TAKE, REFUSE, TAKE),
    'uis_stream_prime': (LEAVE, REFUSE, REFUSE, TAKE),
    'uis_stream_speakers': _OTHER, 'uis_stream_labels': _OTHER, 'uis_stream_end': _OTHER, 'uis_stream_limits': _OTHER,
    'uis_stream_get_limits': _OTHER, 'uis_stream_bindings': _OTHER, 'uis_stream_nbest': _OTHER,
    'uis_stream_posterior': _OTHER, 'uis_stream_commit': _OTHER, 'uis_stream_committed': _OTHER,
    'uis_stream_restart': _OTHER, 'uis_stream_retire': _OTHER, 'uis_stream_export': _OTHER,
    'uis_stream_export_bound': _OTHER, 'uis_stream_import': _OTHER,
    # everything else touches nothing
    'uis_rnn_step': _NONE, 'uis_model_constants': _NONE, 'uis_eval_accuracy': _NONE, 'uis_last_decode_shape': _NONE,
    'uis_last_decode_info': _NONE, 'uis_decode_limits': _NONE, 'uis_frame_bias': _NONE, 'uis_frame_speakers': _NONE,
}
# what the entry point needs before it: no session, a session that has received nothing, one with both windows filled,
# one with an exported utterance and a fresh slot
NEEDS = {name: 'pushed' for name in RULES if name.startswith('uis_stream_')}
NEEDS.update({'uis_stream_begin': 'none', 'uis_stream_prime': 'fresh', 'uis_stream_import': 'blob'})


class _Bench:
  """One decoder, the case's frames, and where the handle stands (a session open or not)."""

  def __init__(self):
    case = golden_util.load_case('tiny_d16')
    self.dec = _capi.Decoder(case['params'])
    self.seqs = [np.ascontiguousarray(s[:N_FRAMES], dtype=np.float64) for s in case['seqs'][:N_UTT]]
    assert [len(s) for s in self.seqs] == [N_FRAMES] * N_UTT
    self.frames = np.concatenate(self.seqs).astype(np.float32)
    self.offsets = np.arange(N_UTT + 1, dtype=np.int64) * N_FRAMES
    self.labels = np.zeros(N_UTT * N_FRAMES, dtype=np.int32)
    self.open = False
    self.blob = None
    self.export_buf = None

  # ---- the state an entry point needs
  def begin(self):
    self.dec.stream_begin(N_UTT, BEAM, WINDOW)
    self.open = True

  def end(self):
    if self.open:
      self.dec.stream_end()
    self.open = False

  def prepare(self, needs):
    self.clear_tables()
    self.end()
    if needs == 'none':
      return
    self.begin()
    if needs == 'pushed':
      self.dec.stream_push(self.seqs)
      self.export_buf = ctypes.create_string_buffer(self.dec.stream_export_bound(0))
    elif needs == 'blob':
      self.dec.stream_push([self.seqs[0], None])
      self.blob = self.dec.stream_export(0)

  # ---- the setters
  def set_table(self, table, n):
    if table == 'limits':
      self.dec.set_limits(np.zeros(n, dtype=np.int32))
    elif table == 'bias':
      self.dec.set_frame_bias(np.full(n, 0.5))
    elif table == 'hint':
      self.dec.set_frame_speakers(np.zeros(n, dtype=np.uint8))
    else:
      self.dec.set_stream_speakers(np.zeros(n, dtype=np.uint8))

  def clear_tables(self):
    self.dec.set_frame_speakers(None)   # (first: uis_stream_speakers refuses a pending one)
    self.dec.set_stream_speakers(None)
    self.dec.set_frame_bias(None)
    self.dec.set_limits(None)

  # ---- the entry points, with valid arguments
  def call(self, name):
    dec, lib, h = self.dec, self.dec._lib, self.dec._handle   # pylint: disable=protected-access
    if name == 'uis_decode':
      dec.decode(self.frames, self.offsets, BEAM, 1, 1)
    elif name == 'uis_decode_f64':
      dec.decode_f64(self.seqs, BEAM, 1, 1)
    elif name == 'uis_decode_device':
      import torch   # pylint: disable=import-outside-toplevel
      d_frames = torch.tensor(self.frames, device='cuda')
      d_labels = torch.zeros(N_UTT * N_FRAMES, dtype=torch.int32, device='cuda')
      d_scores = torch.zeros(N_UTT, dtype=torch.float32, device='cuda')
      torch.cuda.synchronize()
      dec.decode_device(d_frames.data_ptr(), self.offsets, BEAM, 1, 1, d_labels.data_ptr(), d_scores.data_ptr())
      torch.cuda.synchronize()
    elif name == 'uis_score_labels':
      dec.score_labels(self.frames, self.offsets, self.labels)
    elif name == 'uis_score_speakers':
      dec.score_speakers(self.frames, self.offsets, self.labels, 2)
    elif name == 'uis_stream_begin':
      self.open = False
      dec.stream_begin(N_UTT, BEAM, WINDOW)
      self.open = True
    elif name == 'uis_stream_push':
      dec.stream_push([s[:1] for s in self.seqs])
    elif name == 'uis_stream_prime':
      dec.stream_prime(self.seqs, [[0] * N_FRAMES] * N_UTT)
    elif name == 'uis_stream_speakers':   # (a setter under test clears: its own table, and nothing else)
      dec.set_stream_speakers(None)
    elif name == 'uis_stream_labels':
      dec.stream_labels()
    elif name == 'uis_stream_end':
      rc = lib.uis_stream_end(h)
      self.open = self.open and rc != _capi.UIS_OK
      dec._check(rc, 'uis_stream_end')   # pylint: disable=protected-access
    elif name == 'uis_stream_limits':
      dec.stream_set_limits([0] * N_UTT)
    elif name == 'uis_stream_get_limits':
      dec.stream_limits()
    elif name == 'uis_stream_bindings':
      dec.stream_bindings()
    elif name == 'uis_stream_nbest':
      dec.stream_nbest(BEAM)
    elif name == 'uis_stream_posterior':
      dec.stream_posterior()
    elif name == 'uis_stream_commit':
      dec.stream_commit()
    elif name == 'uis_stream_committed':
      dec.stream_committed()
    elif name == 'uis_stream_restart':
      dec.stream_restart([True, False])
    elif name == 'uis_stream_retire':
      dec.stream_retire(clusters=[None] * N_UTT)
    elif name == 'uis_stream_export_bound':
      dec.stream_export_bound(0)
    elif name == 'uis_stream_export':   # (not the wrapper: it asks uis_stream_export_bound first)
      n = ctypes.c_int64(0)
      dec._check(lib.uis_stream_export(h, 0, self.export_buf, len(self.export_buf), ctypes.byref(n)),   # pylint: disable=protected-access
                 'uis_stream_export', ok=(_capi.UIS_OK,))
    elif name == 'uis_stream_import':
      dec.stream_import(1, self.blob)
    elif name == 'uis_rnn_step':
      p = dec.params
      dec.rnn_step(np.zeros(p['observation_dim']), np.zeros((p['rnn_depth'], p['rnn_hidden_size'])))
    elif name == 'uis_model_constants':
      dec.constants()
    elif name == 'uis_eval_accuracy':
      dec.eval_matched(self.labels, self.labels, self.offsets)
    elif name == 'uis_last_decode_shape':
      n, b = ctypes.c_int32(0), ctypes.c_int32(0)
      dec._check(lib.uis_last_decode_shape(h, ctypes.byref(n), ctypes.byref(b)), 'uis_last_decode_shape')   # pylint: disable=protected-access
    elif name == 'uis_last_decode_info':
      dec.last_overflow()
    elif name == 'uis_decode_limits':
      dec.set_limits(None)
    elif name == 'uis_frame_bias':
      dec.set_frame_bias(None)
    elif name == 'uis_frame_speakers':
      dec.set_frame_speakers(None)
    else:
      raise ValueError(name)

  def status(self, call, *args):
    """(status, message) of a call made through the wrappers."""
    try:
      call(*args)
    except _capi.HipLibraryError as err:
      return err.status, str(err)
    return _capi.UIS_OK, ''

  # ---- is the table still pending?
  def pending(self, table):
    gave = (_capi.UIS_ERR_INVALID_ARG, '{} gave {} '.format(SETTER[table], WRONG))
    if table == 'hint' and self.open:
      rc, msg = self.status(self.call, 'uis_stream_committed')
      return rc == _capi.UIS_ERR_UNSUPPORTED and '(uis_frame_speakers)' in msg
    if table == 'stream_tags':
      if not self.open:
        self.begin()
      rc, msg = self.status(self.call, 'uis_stream_push')
    elif table == 'bias' and self.open:
      rc, msg = self.status(self.call, 'uis_stream_push')
    else:
      self.end()
      rc, msg = self.status(self.call, 'uis_decode')
    return rc == gave[0] and gave[1] in msg


@pytest.fixture(scope='module')
def bench():
  b = _Bench()
  yield b
  b.end()
  b.dec.close()


def test_the_table_covers_the_session_calls_of_the_library():
  """Every uis_stream_* symbol the library exports has a row (a new entry point has to pick a rule here, too)."""
  assert {s for s in _capi.EXPORTED_SYMBOLS if s.startswith('uis_stream_')} == {s for s in RULES if s.startswith('uis_stream_')}
  assert {s for s in _capi.EXPORTED_SYMBOLS if s.startswith(('uis_decode', 'uis_score_'))} - {'uis_decode_kernel_table'} <= set(RULES)


@pytest.mark.parametrize('name', sorted(RULES))
def test_every_entry_point_follows_its_rule(bench, name):
  for table, rule in zip(TABLES, RULES[name]):
    if SETTER[table] == name:   # (a setter replaces its own table: nothing to learn)
      continue
    what = (name, table)
    bench.prepare(NEEDS.get(name, 'none'))
    bench.set_table(table, WRONG)
    rc, msg = bench.status(bench.call, name)
    print(what, rule, rc, msg)
    if rule == LEAVE:
      assert rc == _capi.UIS_OK, (what, msg)
    elif rule == TAKE:
      assert rc == _capi.UIS_ERR_INVALID_ARG and '{} gave {} '.format(SETTER[table], WRONG) in msg, (what, msg)
    else:
      assert rc == _capi.UIS_ERR_UNSUPPORTED and name + ' takes no ' in msg and '({})'.format(SETTER[table]) in msg, (what, msg)
    assert bench.pending(table) == (rule == LEAVE), what
    bench.clear_tables()
    bench.end()
