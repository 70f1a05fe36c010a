"""Model-based walks over a live session: operations in an order nobody planned, against the CPU reference.

tests/session_walk.py writes the plans -- pushes of ragged chunks, commits with and without horizons, restarts of
any subset, primes of fresh slots, refused calls, a non-finite frame -- and runs them on tests/commit_ref.py;
tests/test_session_walk_host.py holds that trace to the oracle and asserts the states it reaches.  Here the same
trace is replayed on a _capi.Decoder session, on every session path of each model shape.  After EVERY operation the
operation's own result and every readout of every slot (test_gpu_restart._Session.snapshot, stream_received,
stream_committed) are compared with the trace: integers and float32 bit patterns, exactly.  A failure names the case,
the path, the step, the operation, the slot and the readout.

UIS_COMMIT_TRACE is on throughout: every commit's line (window frames, labels committed, the length of the prior
tables) is the trace's.  A persistent session also shows, in UIS_RESTART_TRACE, that the resident launch left and came
back where include/uisrnn_hip.h says it does.
"""

import numpy as np
import pytest

import session_walk as sw
import test_gpu_hostile as gh
import test_gpu_restart as gr
from uisrnn_amd import _capi

pytestmark = pytest.mark.gpu

PATHS = {'default': 0, 'stepwise': _capi.UIS_FLAG_STEPWISE, 'resident': _capi.UIS_FLAG_RESIDENT,
         'persistent': _capi.UIS_FLAG_PERSISTENT}
KEYS = sw.PER_UTT + ('received', 'committed')
PUSH_KEYS = ('labels', 'scores', 'beam', 'overflow', 'received', 'committed')   # what uis_stream_labels answers


def _lines(err, call):
  return [dict(zip(line.split()[1::2], line.split()[2::2])) for line in err.splitlines() if line.startswith(call + ':')]


def _light_snapshot(session):
  """The readouts that leave a persistent launch on the device: uis_stream_labels (through its mailbox) and the
  beam scores that call leaves with uis_last_decode_info."""
  dec = session.dec
  lab, scores, overflow, status = dec.stream_labels()
  info = np.empty((session.n_utt, session.beam), dtype=np.float32)
  dec._check(dec._lib.uis_last_decode_info(dec._handle, None, info.ctypes.data_as(_capi._fp)), 'info')  # pylint: disable=protected-access
  return {'labels': [session.final[u] + lab[u].tolist() for u in range(session.n_utt)], 'scores': gr._bits(scores).tolist(),   # pylint: disable=protected-access
          'beam': gr._bits(info).tolist(), 'overflow': overflow.tolist(), 'status': (status, _capi.UIS_OK)}   # pylint: disable=protected-access


def _replay(dec, name, path, stay=False):
  """Replay the trace of sw.CASES[name] on `dec`.  stay: after a push only the readouts that do not make a persistent
  launch leave (so that consecutive pushes go through one launch); after everything else, and without `stay` after
  every operation, all of them.  Returns the resident launches the header's rules predict at every restart."""
  tr, case = sw.walk(name), sw.CASES[name]
  n_utt, beam = case['n_utt'], case['beam']
  assert _capi.UIS_ERR_INVALID_ARG == sw.INVALID_ARG
  dec.stream_begin(n_utt, beam, case['window'], max_clusters=case['cap'], flags=PATHS[path])
  launches, running, at_restart = 0, False, []
  try:
    session = gr._Session(dec, n_utt, beam)   # pylint: disable=protected-access
    for i, st in enumerate(tr['steps']):
      what = (name, path, 'step', i, st['op'])
      kind, call, want = st['kind'], st['call'], st['result']
      if kind == 'push':
        dec.stream_push(call['chunks'])
        if any(c is not None for c in call['chunks']) and not running:
          launches, running = launches + 1, True
      elif kind in ('commit_none', 'commit_h'):
        got = session.commit(call['horizons'])
        for u in range(n_utt):
          assert (got[0][u], got[1][u]) == (want['labels'][u], want['dropped'][u]), what + ('slot', u)
        running = running and not sum(want['have'])
      elif kind == 'restart':
        at_restart.append(launches)
        got, status = session.restart({u for u in range(n_utt) if call['which'][u]})
        assert status == _capi.UIS_OK and sorted(got) == sorted(want), what
        for u in want:
          assert got[u] == want[u], what + ('slot', u)
        running = running and not want
      elif kind == 'prime':
        scores = dec.stream_prime(call['chunks'], call['labels'])
        for u in range(n_utt):
          assert int(gr._bits(scores)[u]) == want.get(u, 0), what + ('slot', u)   # pylint: disable=protected-access
        running = False
      else:
        with pytest.raises(_capi.HipLibraryError) as err:
          if call['call'] == 'push':
            dec.stream_push(call['chunks'])
          else:
            dec.stream_prime(call['chunks'], call['labels'])
        assert err.value.status == want, what
      light = stay and kind == 'push'
      shot = _light_snapshot(session) if light else session.snapshot()
      running = running and light
      assert shot['status'] == (_capi.UIS_OK, _capi.UIS_OK), what
      shot['received'], shot['committed'] = dec.stream_received().tolist(), dec.stream_committed().tolist()
      for u in range(n_utt):
        for key in PUSH_KEYS if light else KEYS:
          assert shot[key][u] == st['snap'][u][key], what + ('slot', u, key)
  finally:
    dec.stream_end()
  return at_restart


def _commit_lines(name):
  return [st['result']['line'] for st in sw.walk(name)['steps'] if st['kind'].startswith('commit') and st['result']['line']]


def _check_commit_lines(err, name, runs):
  got = [{k: int(line[k]) for k in ('window_frames', 'committed', 'prior_table_entries')} for line in _lines(err, 'uis_stream_commit')]
  assert got == _commit_lines(name) * runs, name


def _walk_case(name, paths, monkeypatch, capfd):
  monkeypatch.setenv('UIS_COMMIT_TRACE', '1')
  dec = _capi.Decoder(sw.walk(name)['params'])
  for path in paths:
    _replay(dec, name, path)
  dec.close()
  _check_commit_lines(capfd.readouterr().err, name, len(paths))


@pytest.mark.parametrize('name', ['small4', 'small10'])
def test_small(name, oracle_lib, monkeypatch, capfd):
  _walk_case(name, ('default', 'stepwise'), monkeypatch, capfd)


def test_deep(oracle_lib, monkeypatch, capfd):
  _walk_case('deep', ('default', 'stepwise'), monkeypatch, capfd)


def test_embedded(oracle_lib, monkeypatch, capfd):
  _walk_case('embedded', ('default', 'stepwise', 'resident'), monkeypatch, capfd)


def test_one_launch(oracle_lib, monkeypatch, capfd):
  _walk_case('one_launch', ('default', 'resident'), monkeypatch, capfd)


def test_one_launch_persistent(oracle_lib, monkeypatch, capfd):
  """Twice: with every readout after every operation (uis_stream_nbest makes the launch leave: every push starts a
  new one), and with only uis_stream_labels after a push (consecutive pushes stay in one launch; commit, restart and
  prime make it leave; a refused push, a restart of nothing and uis_stream_labels do not)."""
  if not gh._whole_device():   # pylint: disable=protected-access
    pytest.skip('not a whole MI355X')
  name = 'one_launch'
  monkeypatch.setenv('UIS_COMMIT_TRACE', '1')
  monkeypatch.setenv('UIS_RESTART_TRACE', '1')
  monkeypatch.setenv('UIS_PERSIST_IDLE_MS', '2000')   # (the launch must not leave for idleness between two calls)
  dec = _capi.Decoder(sw.walk(name)['params'])
  want = []
  for stay in (False, True):
    want.append(_replay(dec, name, 'persistent', stay=stay))
  dec.close()
  err = capfd.readouterr().err
  _check_commit_lines(err, name, 2)
  steps = sw.walk(name)['steps']
  pushes = [sum(1 for s in steps[:i] if s['kind'] == 'push') for i, s in enumerate(steps) if s['kind'] == 'restart']
  assert want[0] == pushes and want[1] != pushes and all(a <= b for a, b in zip(want[1], pushes)), want
  lines = _lines(err, 'uis_stream_restart')
  assert all(line['persistent'] == '1' for line in lines), lines
  assert [int(line['resident_launches']) for line in lines] == want[0] + want[1], (lines, want)
  assert [int(line['selected']) for line in lines] == [sum(s['call']['which']) for s in steps if s['kind'] == 'restart'] * 2


@pytest.mark.parametrize('word', gr.WORDS)
def test_no_readout_depends_on_stale_memory(word, oracle_lib, monkeypatch):
  monkeypatch.setenv(gr.KNOB, word)
  monkeypatch.delenv('UIS_NO_ARENA', raising=False)
  dec = _capi.Decoder(sw.walk('small4')['params'])
  for path in ('default', 'stepwise'):
    _replay(dec, 'small4', path)
  dec.close()
