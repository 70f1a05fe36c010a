"""tests/policy_walk.py's small plan on a session whose slots carry minimum turn lengths, on the GPU against
tests/turn_walk.py's trace, bit for bit, after every operation: the n-best rows, the scores, uis_session_turns, the
blobs' last-label words, the frame counts, the limits.

The plan is imported and not edited.  It interleaves what tests/test_gpu_turn_session.py holds one by one: pushes under
bias tables (hard ones that empty beams, a non-finite frame, a table left pending by a refusal), commits, retirements
between slots of different values, uis_stream_limits mid-stream, primes, moves from one value to another (the import
normalises the runs), every refusal -- each of which must leave the session as it was.  A slot takes its next value
whenever the plan leaves it fresh.  tests/test_turn_session_host.py asserts what the trace reaches.
"""

import pytest

import test_gpu_turn_session as gts
import turn_walk as tw
from uisrnn_amd import _capi

pytestmark = pytest.mark.gpu


def _refused(call, status, what):
  with pytest.raises(_capi.HipLibraryError) as err:
    call()
  assert err.value.status == status, what


def _replay(dec, path):
  sh, steps = tw.shape(), tw.trace()
  n_utt = sh.n_utt
  assert (_capi.UIS_ERR_INVALID_ARG, _capi.UIS_ERR_UNSUPPORTED) == (tw.INVALID_ARG, tw.UNSUPPORTED)
  dec.stream_begin(n_utt, sh.beam, sh.window, max_clusters=sh.cap, flags=gts.PATHS[path])
  try:
    for i, st in enumerate(steps):
      what = (path, 'step', i) + tuple(st['op'][:2])
      kind, call, want = st['kind'], st['call'], st['result']
      if kind == 'push':
        dec.stream_push(call['chunks'], bias=call['bias'])
      elif kind == 'commit':
        labels, dropped = dec.stream_commit(call['horizons'])
        assert [x.tolist() for x in labels] == want['labels'] and dropped.tolist() == want['dropped'], what
      elif kind == 'restart':
        dec.stream_restart(call['which'])
      elif kind == 'setm':
        dec.session_set_min_turn(call['values'])
        assert dec.session_min_turn().tolist() == call['values'], what
      elif kind == 'prime':
        scores = dec.stream_prime(call['chunks'], call['labels'])
        for u in range(n_utt):
          assert int(gts._bits(scores)[u]) == want.get(u, 0), what + ('slot', u)   # pylint: disable=protected-access
      elif kind == 'limits':
        dec.stream_set_limits(call['limits'])
      elif kind == 'retire':
        res = dec.stream_retire(None, call['clusters'])
        for u in range(n_utt):
          got = (res['retired'][u].tolist(), int(res['K'][u]), res['retirable'][u].tolist())
          assert got == (want['retired'][u], want['K'][u], want['retirable'][u]), what + ('slot', u)
      elif kind == 'move':
        src, dst = call['src'], call['dst']
        blob = dec.stream_export(src)
        assert gts._words(blob) == want['words'], what   # pylint: disable=protected-access
        dec.stream_restart([u == dst for u in range(n_utt)])
        dec.stream_import(dst, blob)
        dec.stream_restart([u == src for u in range(n_utt)])
      elif kind == 'move_refused':
        _refused(lambda: dec.stream_export(call['src']), want, what)   # pylint: disable=cell-var-from-loop
      elif call['call'] == 'push':
        _refused(lambda: dec.stream_push(call['chunks'], bias=call['bias']), want, what)   # pylint: disable=cell-var-from-loop
      elif call['call'] == 'prime':
        if call['bias'] is not None:
          dec.set_frame_bias(call['bias'])
        _refused(lambda: dec.stream_prime(call['chunks'], call['labels']), want, what)   # pylint: disable=cell-var-from-loop
      elif call['call'] == 'limits':
        _refused(lambda: dec.stream_set_limits(call['limits']), want, what)   # pylint: disable=cell-var-from-loop
      else:
        assert call['call'] == 'frame_bias', what
        dec.set_frame_bias(call['stays'])   # stays pending: the next push, which passes no table, runs under it
        _refused(lambda: dec.set_frame_bias(call['bias']), want, what)   # pylint: disable=cell-var-from-loop
      gts._check(dec, sh, st['snap'], what)   # pylint: disable=protected-access
      assert dec.stream_limits().tolist() == [col['limit'] for col in st['snap']], what
      assert dec.session_min_turn().tolist() == [col['m'] for col in st['snap']], what
  finally:
    dec.stream_end()


@pytest.mark.parametrize('path', ['default', 'stepwise'])
def test_the_policy_walks_small_plan_under_slot_values(path, oracle_lib):
  dec = _capi.Decoder(tw.shape().params)
  try:
    _replay(dec, path)
  finally:
    dec.close()
