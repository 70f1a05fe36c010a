"""Device tensors in, end to end: predict_tensors against predict, sessions fed by push_tensors against sessions fed by
push -- bit for bit, because everything behind the packed float32 stream is shared and tests/test_gpu_ingest.py holds
the stream itself to the reference.

 1. predict_tensors == predict (labels; scores against the decode of the same float64 arrays) for float64, float32,
    float16 and bfloat16 -- the three narrower ones against predict of the exactly upcast arrays -- on a launch-per-step
    shape (tiny_d16) and a one-launch shape (k_decode_rs, 256 x 256, tests/instantiation_cases.py); an empty utterance in
    the list, the [U, T, D] + lengths form, a single [N, D] tensor, one call carrying all four rule tables
 2. a session fed by push_tensors in three chunkings (one frame, ragged, everything at once) against the same session
    fed by push: labels, scores and the exported blob bytes of every slot, on the launch-per-step path, the one-launch
    path and under UIS_POISON_WORKSPACE; a pending bias / speaker table applies as in push
 3. OnlineSession.push_tensors and StreamPool.push_tensors against push, with names and a commit horizon
 4. a persistent session refuses tensors and stays as it was
 5. a tensor written on a side stream immediately before the call
 6. both shapes under UIS_FLAG_STEPWISE (tiny_d16's own choice is its one-workgroup kernel), through decode_tensors
 7. uis_tensors_decode takes and consumes the per-call tables by the decode's rule, and refuses bad lists
"""

import numpy as np
import pytest
import torch

import golden_util
import instantiation_cases as ic
import test_gpu_hostile as gh
import uisrnn_amd
from uisrnn_amd import _capi

pytestmark = pytest.mark.gpu

DTYPES = (torch.float64, torch.float32, torch.float16, torch.bfloat16)
KNOB = 'UIS_POISON_WORKSPACE'
RS_ROW = (ic.RS, 256, 256, ic.RS_BASE, 0)


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _name(dtype):
  return str(dtype).split('.')[1]


def _ncl():
  n_cu = torch.cuda.get_device_properties(0).multi_processor_count
  return n_cu // 32 if n_cu >= 32 and n_cu % 32 == 0 and n_cu // 32 <= 16 else 0


def _shape(name):
  """(params, float64 utterances, beam, cap, test_iteration, whether the shape has a one-launch cluster kernel)."""
  if name == 'tiny_d16':
    case = golden_util.load_case('tiny_d16')
    return case['params'], [np.asarray(s, dtype=np.float64) for s in case['seqs']], 4, 16, 2, False
  ncl = _ncl()
  if ncl == 0:
    pytest.skip('no cluster of 32 compute units: the one-launch kernels do not apply')
  case = ic.CASES[RS_ROW][0]
  return case.params(), [np.asarray(s, dtype=np.float64) for s in case.utterances(ncl)], case.beam, case.cap, 2, True


def _model(params, beam, cap, test_iteration):
  model_args, _, args = uisrnn_amd.parse_arguments([])
  model_args.observation_dim = int(params['observation_dim'])
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params)
  args.beam_size, args.look_ahead, args.test_iteration, args.max_clusters = beam, 1, test_iteration, cap
  return model, args


def _device(seqs, dtype):
  """The utterances as device tensors of `dtype`, and the float64 arrays that hold exactly their values."""
  tensors = [torch.from_numpy(s).to(dtype).cuda() for s in seqs]
  return tensors, [t.double().cpu().numpy() for t in tensors]


# ---- 1. predict_tensors against predict

@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
@pytest.mark.parametrize('name', ['tiny_d16', 'rs_256x256'])
def test_predict_tensors_equals_predict(name, dtype):
  params, seqs, beam, cap, tau, clustered = _shape(name)
  dim = seqs[0].shape[1]
  seqs = seqs[:2] + [np.zeros((0, dim))] + seqs[2:]   # an empty utterance in the list
  model, args = _model(params, beam, cap, tau)
  tensors, exact = _device(seqs, dtype)
  want = model.predict(exact, args)
  want_scores = model._get_decoder().decode_f64(exact, beam, 1, tau, max_clusters=cap)['scores']  # pylint: disable=protected-access
  labels, scores = model.predict_tensors(tensors, args, return_scores=True)
  if clustered:   # (what predict reports for this shape: tests/test_gpu_instantiations.py)
    assert model.last_stats['decode_kernel'] in ('k_decode_rs', 'k_decode_resident'), model.last_stats['decode_kernel']
  assert all(lab.dtype == torch.int32 and lab.is_cuda for lab in labels)
  assert [lab.tolist() for lab in labels] == want
  assert np.array_equal(_bits(scores), _bits(want_scores))
  base = labels[0].untyped_storage().data_ptr()
  assert all(lab.untyped_storage().data_ptr() == base for lab in labels)   # views of one label tensor
  assert model.predict_tensors(tensors, args)[3].tolist() == want[3]
  # a single [N, D] tensor; a view of a wider tensor; the padded batch with lengths
  one, score = model.predict_tensors(tensors[0], args, return_scores=True)
  assert one.tolist() == want[0] and _bits(score) == _bits(want_scores[0])
  wide = torch.cat([tensors[1], tensors[1] + 1], dim=1)
  assert model.predict_tensors(wide[:, :dim], args).tolist() == want[1]
  most = max(len(s) for s in seqs)
  batch = torch.full((len(seqs), most, dim), float('nan'), dtype=dtype, device='cuda')   # (what lies behind a length is never read)
  for u, t in enumerate(tensors):
    batch[u, :len(t)] = t
  lengths = [len(s) for s in seqs]
  got, got_scores = model.predict_tensors(batch, args, lengths=lengths, return_scores=True)
  assert [lab.tolist() for lab in got] == want and np.array_equal(_bits(got_scores), _bits(want_scores))
  got = model.predict_tensors(batch, args, lengths=torch.tensor(lengths))
  assert [lab.tolist() for lab in got] == want


@pytest.mark.parametrize('name', ['tiny_d16', 'rs_256x256'])
def test_one_call_carrying_all_four_rule_tables(name):
  params, seqs, beam, cap, tau, _ = _shape(name)
  seqs = seqs[:4]
  model, args = _model(params, beam, cap, tau)
  tensors, exact = _device(seqs, torch.float16)
  rng = np.random.default_rng(5)
  rules = dict(max_speakers=[3, 0, 2, 4][:len(seqs)],
               transition_bias=[np.where(rng.random(len(s)) < 0.3, np.nan, rng.random(len(s)) * 0.8 + 0.1) for s in seqs],
               # (a turn every three frames: no contradiction with min_turn 3 and max_speakers 2)
               known_speakers=[[('a' if t % 6 == 0 else 'b' if t % 6 == 3 else None) for t in range(len(s))] for s in seqs],
               min_turn=[2, 0, 3, 1][:len(seqs)])
  free = model.predict(exact, args)
  want = model.predict(exact, args, **rules)
  assert want != free   # (the tables bind)
  got = model.predict_tensors(tensors, args, **rules)
  assert [lab.tolist() for lab in got] == want
  # the tables were this call's: the next one decodes without them
  assert [lab.tolist() for lab in model.predict_tensors(tensors, args)] == free


# ---- 2. sessions: push_tensors against push

def _chunkings(seqs, case_pushes):
  lens = [len(s) for s in seqs]
  one = [[1 if t < n else 0 for n in lens] for t in range(max(lens))]
  return {'one frame': one, 'ragged': case_pushes, 'at once': [lens]}


def _run_session(dec, seqs, pushes, beam, cap, flags, tensors=None, tables=None):
  """Labels, scores, overflow words and every slot's exported blob after the pushes; tensors: the utterances as device
  tensors (push_tensors) or None (push of the float32 arrays).  tables: {push index: {'bias': .., 'speakers': ..}}."""
  dec.stream_begin(len(seqs), beam, max(len(s) for s in seqs), max_clusters=cap, flags=flags)
  try:
    pos = [0] * len(seqs)
    for i, take in enumerate(pushes):
      extra = (tables or {}).get(i, {})
      if tensors is None:
        dec.stream_push([np.asarray(s[p:p + n], dtype=np.float32) if n else None for s, p, n in zip(seqs, pos, take)], **extra)
      else:
        dec.stream_push_tensors([t[p:p + n] if n else None for t, p, n in zip(tensors, pos, take)], **extra)
      pos = [p + n for p, n in zip(pos, take)]
    assert dec.stream_received().tolist() == [len(s) for s in seqs]
    labels, scores, overflow, status = dec.stream_labels()
    blobs = [bytes(dec.stream_export(u)) for u in range(len(seqs))]
  finally:
    dec.stream_end()
  assert status == 0
  return [lab.tolist() for lab in labels], _bits(scores).tolist(), overflow.tolist(), blobs


def _session_shape(path):
  if path == 'stepwise':
    case = golden_util.load_case('tiny_d16')
    seqs = [np.asarray(s, dtype=np.float64) for s in case['seqs']]
    lens = [len(s) for s in seqs]
    sizes, left, ragged, k = (1, 7, 3, 16, 5, 2, 11), list(lens), [], 0
    while any(left):
      take = [min(sizes[(k + u) % len(sizes)], n) for u, n in enumerate(left)]
      left = [n - t for n, t in zip(left, take)]
      ragged.append(take)
      k += 1
    return case['params'], seqs, ragged, 4, 16, _capi.UIS_FLAG_STEPWISE
  ncl = _ncl()
  if ncl == 0:
    pytest.skip('no cluster of 32 compute units: the one-launch kernels do not apply')
  case = ic.CASES[RS_ROW][0]
  seqs = [np.asarray(s, dtype=np.float64) for s in case.utterances(ncl)]
  return case.params(), seqs, case.pushes(ncl), case.beam, case.cap, _capi.UIS_FLAG_RESIDENT


@pytest.mark.parametrize('chunking,dtype', [('one frame', torch.float64), ('ragged', torch.float16), ('at once', torch.float32),
                                            ('ragged', torch.bfloat16)], ids=lambda v: v if isinstance(v, str) else _name(v))
@pytest.mark.parametrize('path', ['stepwise', 'resident', 'poison'])
def test_a_session_fed_by_push_tensors_is_the_session_fed_by_push(path, chunking, dtype, monkeypatch):
  """Labels, scores and the exported blob bytes of every slot.  'poison': the one-launch shape under
  UIS_POISON_WORKSPACE with the library's own choice of path per push (both kinds of push occur)."""
  params, seqs, ragged, beam, cap, flags = _session_shape('resident' if path == 'poison' else path)
  if path == 'poison':
    monkeypatch.setenv(KNOB, 'ffffffff')
    flags = 0
  tensors, exact = _device(seqs, dtype)
  pushes = _chunkings(seqs, ragged)[chunking]
  dec = _capi.Decoder(params)
  try:
    want = _run_session(dec, exact, pushes, beam, cap, flags)
    picked = dec.last_instantiation()[0]
    got = _run_session(dec, exact, pushes, beam, cap, flags, tensors=tensors)
    assert dec.last_instantiation()[0] == picked
    if path != 'poison':
      assert picked == ('stepwise' if path == 'stepwise' else 'k_decode_resident')
  finally:
    dec.close()
  assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]
  for u, (a, b) in enumerate(zip(got[3], want[3])):
    assert a == b, ('blob of slot', u)


@pytest.mark.parametrize('path', ['stepwise', 'resident'])
def test_a_pending_bias_and_speaker_table_apply_as_in_push(path):
  params, seqs, ragged, beam, cap, flags = _session_shape(path)
  tensors, exact = _device(seqs, torch.float32)
  rng = np.random.default_rng(9)
  tables = {}
  for i, take in enumerate(ragged):
    n = sum(take)
    if n and i % 2 == 0:
      tables[i] = {'bias': np.where(rng.random(n) < 0.5, np.nan, rng.random(n) * 0.8 + 0.1),
                   'speakers': (rng.random(n) < 0.3).astype(np.uint8) * rng.integers(1, 3, n).astype(np.uint8)}
  dec = _capi.Decoder(params)
  try:
    free = _run_session(dec, exact, ragged, beam, cap, flags)
    want = _run_session(dec, exact, ragged, beam, cap, flags, tables=tables)
    got = _run_session(dec, exact, ragged, beam, cap, flags, tensors=tensors, tables=tables)
    # a table of the wrong length is refused as in push, the session untouched, and the table consumed
    dec.stream_begin(len(seqs), beam, 8, max_clusters=cap, flags=flags)
    try:
      dec.set_frame_bias(np.full(len(seqs) + 1, 0.5))
      with pytest.raises(_capi.HipLibraryError) as err:
        dec.stream_push_tensors([t[:1] for t in tensors])
      assert err.value.status == _capi.UIS_ERR_INVALID_ARG and 'uis_frame_bias gave' in str(err.value)
      assert dec.stream_received().tolist() == [0] * len(seqs)
      dec.stream_push_tensors([t[:1] for t in tensors])
      # an utterance beyond the session's window, and a list of the wrong length
      with pytest.raises(_capi.HipLibraryError) as err:
        dec.stream_push_tensors([torch.cat([t[:4], t[:4]]) for t in tensors])
      assert err.value.status == _capi.UIS_ERR_INVALID_ARG and 'max_frames' in str(err.value)
      with pytest.raises(ValueError):
        dec.stream_push_tensors(tensors[:-1])
      assert dec.stream_received().tolist() == [1] * len(seqs)
    finally:
      dec.stream_end()
  finally:
    dec.close()
  assert want != free and got == want


# ---- 3. the Python sessions

def test_online_session_and_pool_push_tensors_against_push():
  params, seqs, _, beam, cap, _ = _session_shape('stepwise')
  seqs = seqs[:3]
  model, args = _model(params, beam, cap, 1)
  tensors, exact = _device(seqs, torch.float16)
  n = min(len(s) for s in seqs)
  names = [[('ann' if t % 4 == 0 else None) for t in range(n)] for _ in seqs]
  bias = [np.full(n, 0.25) for _ in seqs]

  def feed(push, data, block):
    if block:   # the [U, n, D] form in two pushes
      push(data[:, :3], transition_bias=np.stack(bias)[:, :3])
      push(data[:, 3:], known_speakers=[row[3:] for row in names])
    else:
      push([d[:3] for d in data], transition_bias=[b[:3] for b in bias])
      push([data[0][3:n], None, data[2][3:n]], known_speakers=[names[0][3:], None, names[2][3:]])
      push([None, data[1][3:n], None], known_speakers=[None, names[1][3:], None])

  results = []
  for block in (False, True):
    for device in (False, True):
      with model.online(3, args, max_frames=n + 1, horizon=4) as session:
        if device:
          data = torch.stack([t[:n] for t in tensors]) if block else tensors
          feed(session.push_tensors, data, block)
        else:
          data = np.stack([s[:n] for s in exact]) if block else exact
          feed(session.push, data, block)
        results.append((session.labels(), session.speakers(), [bytes(session.export_state(u)) for u in range(3)]))
  assert results[0] == results[1] and results[2] == results[3]
  # a pool: keys to slots, then OnlineSession.push_tensors
  out = []
  for device in (False, True):
    with model.online_pool(3, args, max_frames=n + 1) as pool:
      pool.open('x')
      pool.open('y')
      data = tensors if device else exact
      (pool.push_tensors if device else pool.push)({'y': data[1][:5], 'x': data[0][:2]}, known_speakers={'y': ['bob'] * 5})
      (pool.push_tensors if device else pool.push)({'x': data[0][2:6]})
      out.append((pool.labels('x'), pool.labels('y'), pool.speakers('y')))
  assert out[0] == out[1]
  # what is no device tensor of the model's width is refused before the library, the session untouched
  with model.online(3, args, max_frames=8) as session:
    for bad, error in (([t.cpu()[:2] for t in tensors], TypeError), ([t[:2].to(torch.int32) for t in tensors], TypeError),
                       ([e[:2] for e in exact], TypeError), ([t[:2, :3] for t in tensors], ValueError),
                       ([t[:2] for t in tensors][:2], ValueError)):
      with pytest.raises(error):
        session.push_tensors(bad)
    assert session._decoder.stream_received().tolist() == [0, 0, 0]   # pylint: disable=protected-access
    session.push_tensors([t[:2] for t in tensors])
    assert [len(x) for x in session.labels()] == [2, 2, 2]


# ---- 4. a persistent session

def test_a_persistent_session_refuses_tensors_and_stays_as_it_was():
  if not gh._whole_device():   # pylint: disable=protected-access
    pytest.skip('not a whole MI355X')
  case = ic.CASES[(ic.RESIDENT, 256, 256, ic.CLS_NONE, 1)][0]
  ncl = _ncl()
  seqs = [np.asarray(s, dtype=np.float64) for s in case.utterances(ncl)]
  tensors, exact = _device(seqs, torch.float32)
  pushes = case.pushes(ncl)   # (at most 16 frames an utterance: every push goes through the mailbox)
  dec = _capi.Decoder(case.params())
  try:
    dec.stream_begin(len(seqs), case.beam, max(len(s) for s in seqs), max_clusters=case.cap, flags=_capi.UIS_FLAG_PERSISTENT)
    try:
      pos = [0] * len(seqs)
      for i, take in enumerate(pushes):
        if i == 1:   # between two pushes of the running launch
          before = dec.stream_received()
          with pytest.raises(_capi.HipLibraryError) as err:
            dec.stream_push_tensors([t[p:p + n] if n else None for t, p, n in zip(tensors, pos, take)])
          assert err.value.status == _capi.UIS_ERR_UNSUPPORTED and 'UIS_FLAG_PERSISTENT' in str(err.value)
          assert dec.stream_received().tolist() == before.tolist() and before.sum() > 0
        dec.stream_push([np.asarray(s[p:p + n], dtype=np.float32) if n else None for s, p, n in zip(exact, pos, take)])
        assert dec.last_instantiation()[4] == 1   # (still the launch that stays)
        pos = [p + n for p, n in zip(pos, take)]
      labels = [lab.tolist() for lab in dec.stream_labels()[0]]
    finally:
      dec.stream_end()
    want = _run_session(dec, exact, [[len(s) for s in seqs]], case.beam, case.cap, 0)
    assert labels == want[0]
  finally:
    dec.close()
  # the Python session says so at once
  model, args = _model(case.params(), case.beam, case.cap, 1)
  with model.online(len(seqs), args, max_frames=8, persistent=True) as session:
    assert session.persistent
    with pytest.raises(ValueError, match='persistent'):
      session.push_tensors([t[:1] for t in tensors])
    session.push([s[:1] for s in exact])
    assert [len(x) for x in session.labels()] == [1] * len(seqs)


# ---- 5. ordering behind the producer's stream

def test_a_tensor_written_on_a_side_stream_just_before_the_call():
  """The utterances are written by a torch op on a side stream, behind enough queued work that the write has not
  happened when predict_tensors is entered; the call is made with that stream current, so the library must wait for
  it (an event recorded there) before k_ingest reads.  Without the wait the gather would read the buffer's earlier
  contents and the labels would differ -- usually: this test CAN pass by luck without the event wait, if the side
  stream happens to drain first; it cannot fail with it."""
  params, seqs, beam, cap, tau, _ = _shape('tiny_d16')
  model, args = _model(params, beam, cap, tau)
  tensors, exact = _device(seqs, torch.float32)
  want = model.predict(exact, args)
  assert [lab.tolist() for lab in model.predict_tensors(tensors, args)] == want   # (warm: handles, workspaces)
  stale = [torch.zeros_like(t) for t in tensors]
  side = torch.cuda.Stream()
  a = torch.randn(4096, 4096, device='cuda')
  torch.cuda.synchronize()
  with torch.cuda.stream(side):
    for _ in range(20):
      a = (a @ a).clamp_(-1, 1)                # tens of milliseconds of queued work
    for s, t in zip(stale, tensors):
      s.copy_(t, non_blocking=True)            # ... behind which the utterances are written
    got = model.predict_tensors(stale, args)   # (torch's current stream is the side stream: the producer)
  assert [lab.tolist() for lab in got] == want
  # ... and named explicitly, from the default stream
  dec = model._get_decoder()   # pylint: disable=protected-access
  again = [torch.zeros_like(t) for t in tensors]
  with torch.cuda.stream(side):
    for _ in range(20):
      a = (a @ a).clamp_(-1, 1)
    for s, t in zip(again, tensors):
      s.copy_(t, non_blocking=True)
  out = dec.decode_tensors(again, beam, 1, tau, max_clusters=cap, stream=side.cuda_stream)
  side.synchronize()
  offsets = np.cumsum([0] + [len(s) for s in seqs])
  assert [out['labels'][offsets[u]:offsets[u + 1]].tolist() for u in range(len(seqs))] == want


# ---- 6. and 7. the C entry: the launch-per-step path, its rule and its refusals

@pytest.mark.parametrize('name', ['tiny_d16', 'rs_256x256'])
def test_the_launch_per_step_path_from_tensors(name):
  """UIS_FLAG_STEPWISE, which predict_tensors has no word for: the four kernels per step behind the gathered stream."""
  params, seqs, beam, cap, tau, _ = _shape(name)
  tensors, exact = _device(seqs, torch.bfloat16)
  dec = _capi.Decoder(params)
  try:
    got = dec.decode_tensors(tensors, beam, 1, tau, max_clusters=cap, flags=_capi.UIS_FLAG_STEPWISE, want_beam_scores=True)
    assert got['stats']['decode_kernel'].startswith('stepwise') and dec.last_instantiation()[0] == 'stepwise'
    want = dec.decode_f64(exact, beam, 1, tau, max_clusters=cap, flags=_capi.UIS_FLAG_STEPWISE, want_beam_scores=True)
  finally:
    dec.close()
  assert got['labels'].tolist() == want['labels'].tolist() and np.array_equal(_bits(got['scores']), _bits(want['scores']))
  assert np.array_equal(_bits(got['beam_scores']), _bits(want['beam_scores']))


def test_uis_tensors_decode_takes_the_decodes_tables_and_refuses_bad_lists():
  params, seqs, beam, cap, tau, _ = _shape('tiny_d16')
  tensors, exact = _device(seqs[:2], torch.float64)
  frames = sum(len(s) for s in exact)
  dec = _capi.Decoder(params)
  try:
    plain = dec.decode_tensors(tensors, beam, 1, tau, max_clusters=cap, want_beam_scores=True)
    host = dec.decode_f64(exact, beam, 1, tau, max_clusters=cap, want_beam_scores=True)
    assert plain['labels'].tolist() == host['labels'].tolist()
    assert np.array_equal(_bits(plain['scores']), _bits(host['scores']))
    assert np.array_equal(_bits(plain['beam_scores']), _bits(host['beam_scores']))   # (uis_last_decode_info is valid)
    assert not plain['empty'].any() and torch.equal(plain['scores_device'].cpu(), torch.from_numpy(plain['scores']))
    nbest = dec.last_nbest(2)
    assert nbest['labels'][0][0].tolist() == plain['labels'][:len(exact[0])].tolist()
    # every table of the decode's rule is taken: a wrong count is this call's refusal, and the table is gone afterwards
    for setter, wrong, text in ((dec.set_limits, np.zeros(7, dtype=np.int32), 'uis_decode_limits gave 7'),
                                (dec.set_min_turn, np.zeros(7, dtype=np.int32), 'uis_min_turn gave 7'),
                                (dec.set_frame_bias, np.full(frames + 1, 0.5), 'uis_frame_bias gave'),
                                (dec.set_frame_speakers, np.zeros(frames + 1, dtype=np.uint8), 'uis_frame_speakers gave')):
      setter(wrong)
      with pytest.raises(_capi.HipLibraryError) as err:
        dec.decode_tensors(tensors, beam, 1, tau, max_clusters=cap)
      assert err.value.status == _capi.UIS_ERR_INVALID_ARG and text in str(err.value)
      assert dec._lib.uis_last_decode_shape(dec._handle, None, None) == 0   # pylint: disable=protected-access
      again = dec.decode_tensors(tensors, beam, 1, tau, max_clusters=cap)
      assert again['labels'].tolist() == host['labels'].tolist()
    # an open session refuses the decode, as its siblings
    dec.stream_begin(2, beam, 8, max_clusters=cap)
    try:
      with pytest.raises(_capi.HipLibraryError) as err:
        dec.decode_tensors(tensors, beam, 1, tau, max_clusters=cap)
      assert err.value.status == _capi.UIS_ERR_INVALID_ARG and 'session' in str(err.value)
    finally:
      dec.stream_end()
    # an empty list
    none = dec.decode_tensors([], beam, 1, tau, max_clusters=cap)
    assert none['labels'].numel() == 0 and none['scores'].shape == (0,)
  finally:
    dec.close()
