"""Model-based walks over a live session under speaker bounds (uis_stream_limits) and per-frame turn priors
(uis_frame_bias before uis_stream_push), against the CPU reference.

tests/policy_walk.py writes the plans -- pushes whose slots carry tables of different kinds or none, limits raised,
lowered below a live K, set to 0 and to the cap, retirements, moves between slots of different limits (export, restart,
import, restart), commits, restarts, primes, both contradictions, every refusal that consumes a table -- and runs them
on tests/bias_ref.py; tests/test_policy_walk_host.py ties that trace to the oracle and asserts the states it reaches.
Here the trace is replayed on a _capi.Decoder session, on every session path of each model shape.  After EVERY
operation the operation's own result, every readout of every slot (test_gpu_restart._Session.snapshot,
stream_received, stream_committed) and stream_limits() are compared with the trace: integers and float32 bit patterns,
exactly.  A failure names the case, the path, the step, the operation, the slot and the readout.
"""

import pytest

import policy_walk as pw
import test_gpu_hostile as gh
import test_gpu_restart as gr
import test_gpu_session_walk as gw
import uisrnn_amd
from uisrnn_amd import _capi

pytestmark = pytest.mark.gpu

PATHS = gw.PATHS
PUSH_KEYS = gw.PUSH_KEYS + ('limit',)


def _refused(call, status, what):
  with pytest.raises(_capi.HipLibraryError) as err:
    call()
  assert err.value.status == status, what


def _restarted(session, u, want, what):
  got, status = session.restart({u})
  assert status == _capi.UIS_OK and got == {u: want}, what + ('slot', u)


def _replay(dec, name, path, stay=False):
  """Replay the trace of pw.CASES[name] on `dec`.  stay: after a push only the readouts that do not make a persistent
  launch leave."""
  tr, case = pw.walk(name), pw.CASES[name]
  n_utt, beam = case['n_utt'], case['beam']
  assert (_capi.UIS_ERR_INVALID_ARG, _capi.UIS_ERR_UNSUPPORTED) == (pw.INVALID_ARG, pw.UNSUPPORTED)
  dec.stream_begin(n_utt, beam, case['window'], max_clusters=case['cap'], flags=PATHS[path])
  try:
    session = gr._Session(dec, n_utt, beam)   # pylint: disable=protected-access
    for i, st in enumerate(tr['steps']):
      what = (name, path, 'step', i, st['op'][:2])
      kind, call, want = st['kind'], st['call'], st['result']
      if kind == 'push':
        dec.stream_push(call['chunks'], bias=call['bias'])
      elif kind in ('commit_none', 'commit_h'):
        got = session.commit(call['horizons'])
        for u in range(n_utt):
          assert (got[0][u], got[1][u]) == (want['labels'][u], want['dropped'][u]), what + ('slot', u)
      elif kind == 'restart':
        got, status = session.restart({u for u in range(n_utt) if call['which'][u]})
        assert status == _capi.UIS_OK and sorted(got) == sorted(want), what
        for u in want:
          assert got[u] == want[u], what + ('slot', u)
      elif kind == 'prime':
        scores = dec.stream_prime(call['chunks'], call['labels'])
        for u in range(n_utt):
          assert int(gr._bits(scores)[u]) == want.get(u, 0), what + ('slot', u)   # pylint: disable=protected-access
      elif kind == 'limits':
        dec.stream_set_limits(call['limits'])
      elif kind == 'retire':
        res = dec.stream_retire(call['which'], call['clusters'])
        for u in range(n_utt):
          got = (res['retired'][u].tolist(), int(res['K'][u]), res['retirable'][u].tolist())
          assert got == (want['retired'][u], want['K'][u], want['retirable'][u]), what + ('slot', u)
      elif kind == 'move':
        src, dst = call['src'], call['dst']
        blob = dec.stream_export(src)
        _restarted(session, dst, want[dst], what)
        dec.stream_import(dst, blob)
        session.final[dst] = list(session.final[src])   # (the caller keeps the committed labels: they move with it)
        _restarted(session, src, want[src], what)
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
      light = stay and kind == 'push'
      shot = gw._light_snapshot(session) if light else session.snapshot()   # pylint: disable=protected-access
      assert shot['status'] == (_capi.UIS_OK, _capi.UIS_OK), what
      shot['received'], shot['committed'] = dec.stream_received().tolist(), dec.stream_committed().tolist()
      shot['limit'] = dec.stream_limits().tolist()
      for u in range(n_utt):
        for key in PUSH_KEYS if light else pw.KEYS:
          assert shot[key][u] == st['snap'][u][key], what + ('slot', u, key)
  finally:
    dec.stream_end()


def _walk_case(name, paths):
  dec = _capi.Decoder(pw.walk(name)['params'])
  try:
    for path in paths:
      _replay(dec, name, path)
  finally:
    dec.close()


@pytest.mark.parametrize('name', ['small4', 'small10'])
def test_small(name, oracle_lib):
  _walk_case(name, ('default', 'stepwise'))


def test_deep(oracle_lib):
  _walk_case('deep', ('default', 'stepwise'))


def test_embedded(oracle_lib):
  _walk_case('embedded', ('default', 'stepwise', 'resident'))


def test_one_launch(oracle_lib):
  _walk_case('one_launch', ('default', 'resident'))


def test_limits_only_persistent(oracle_lib, monkeypatch):
  """The script without tables on the path that takes none, twice: with every readout after every operation, and with
  only uis_stream_labels after a push (consecutive pushes stay in one launch).  Its one table is refused with
  UIS_ERR_UNSUPPORTED, the snapshot stays and the next push decodes."""
  if not gh._whole_device():   # pylint: disable=protected-access
    pytest.skip('not a whole MI355X')
  monkeypatch.setenv('UIS_PERSIST_IDLE_MS', '2000')   # (the launch must not leave for idleness between two calls)
  steps = pw.walk('limits_only')['steps']
  assert [st['result'] for st in steps if st['op'][:2] == ('refuse', 'bias_push_persistent')] == [_capi.UIS_ERR_UNSUPPORTED]
  dec = _capi.Decoder(pw.walk('limits_only')['params'])
  try:
    for stay in (False, True):
      _replay(dec, 'limits_only', 'persistent', stay=stay)
  finally:
    dec.close()


@pytest.mark.parametrize('word', gr.WORDS)
def test_no_readout_depends_on_stale_memory(word, oracle_lib, monkeypatch):
  """chunk_bias is poisoned at every push: a push without a table behind one with a table must not see it."""
  monkeypatch.setenv(gr.KNOB, word)
  monkeypatch.delenv('UIS_NO_ARENA', raising=False)
  _walk_case('small4', ('default', 'stepwise'))


# ---- the Python entries: labels only (the replays above hold the bits)

def _python_prefix():
  """The leading steps of small4 that OnlineSession has a method for: up to its first move."""
  steps = pw.walk('small4')['steps']
  stop = next(i for i, st in enumerate(steps) if st['kind'] in ('move', 'refuse', 'prime', 'move_refused'))
  head = steps[:stop]
  assert head[0]['kind'] == 'limits' and {'push', 'limits', 'commit_h', 'retire'} <= {st['kind'] for st in head}
  assert sum(st['kind'] == 'push' and st['call']['bias'] is not None for st in head) >= 3
  assert sum(len(r) for st in head if st['kind'] == 'retire' for r in st['result']['retired']) >= 1
  # a bound lifted from live clusters: set_max_speakers takes the 0 and max_speakers() answers None
  assert any(st['kind'] == 'limits' and new == 0 < old and st['aux']['K'][u] > 0
             for st in head[1:] for u, (old, new) in enumerate(zip(st['aux'].get('old', ()), st['call'].get('limits', ()))))
  return head


def _model():
  case = pw.CASES['small4']
  params = pw.walk('small4')['params']
  model_args, _, inference_args = uisrnn_amd.parse_arguments([])
  model_args.observation_dim, model_args.rnn_hidden_size = int(params['observation_dim']), int(params['rnn_hidden_size'])
  model_args.rnn_depth = int(params['rnn_depth'])
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params)
  inference_args.beam_size, inference_args.look_ahead, inference_args.test_iteration = case['beam'], 1, 1
  inference_args.max_clusters = case['cap']
  return model, inference_args


def _python_tables(st):
  """The push's tables as OnlineSession.push takes them: one array or None per slot, or None for all."""
  per = [None if st['aux']['kinds'][u] in (None, 'none') else st['aux']['tables'][u] for u in range(len(st['call']['chunks']))]
  return per if any(t is not None for t in per) else None


def _python_step(session, st, push):
  kind, call = st['kind'], st['call']
  n_utt = len(st['snap'])
  if kind == 'push':
    push(call['chunks'], _python_tables(st))
  elif kind == 'limits':
    session.set_max_speakers(call['limits'])
  elif kind in ('commit_none', 'commit_h'):
    session.commit(None if call['horizons'] is None else [None if h < 0 else h for h in call['horizons']])
  elif kind == 'retire' and any(st['result']['retired']):
    assert call['clusters'] is None
    session.retire(None if call['which'] is None else [u for u in range(n_utt) if call['which'][u]])
  elif kind == 'restart':
    session.restart([u for u in range(n_utt) if call['which'][u]])
  assert session.max_speakers() == [c['limit'] or None for c in st['snap']]
  assert session.labels() == st['aux']['stream_labels'], (st['op'][:2],)


def test_the_online_session_follows_the_walk(oracle_lib):
  head = _python_prefix()
  case = pw.CASES['small4']
  model, args = _model()
  with model.online(case['n_utt'], args, case['window'], max_speakers=head[0]['call']['limits']) as session:
    for st in head[1:]:
      _python_step(session, st, lambda chunks, tables: session.push(chunks, transition_bias=tables))


def test_the_stream_pool_follows_the_walk(oracle_lib):
  head = _python_prefix()
  case = pw.CASES['small4']
  model, args = _model()
  keys = ['call-%d' % u for u in range(case['n_utt'])]
  with model.online_pool(case['n_utt'], args, case['window']) as pool:
    for u, key in enumerate(keys):
      assert pool.open(key, max_speakers=head[0]['call']['limits'][u]) == u

    def push(chunks, tables):
      bias = None if tables is None else {keys[u]: t for u, t in enumerate(tables) if t is not None}
      pool.push({keys[u]: c for u, c in enumerate(chunks) if c is not None}, transition_bias=bias)

    for st in head[1:]:
      _python_step(pool._session, st, push)   # pylint: disable=protected-access
    assert [pool.labels(key) for key in keys] == head[-1]['aux']['stream_labels']
