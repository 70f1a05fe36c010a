"""Known speakers in streaming sessions (uis_stream_speakers, uis_stream_bindings) on the GPU against
tests/known_session_ref.py, bit for bit: the n-best rows, the scores, the final beam, the bindings.

Shapes are tests/session_walk.py's; the plans and their traces on the CPU reference are tests/known_session_cases.py's
(computed once, shared, never written to; tests/test_known_session_host.py asserts what they are meant to reach: the
tags change the labels, no beam empties, no cap is in reach, the retire case holds both kinds of cluster).  Every case
runs under UIS_FLAG_STEPWISE and UIS_FLAG_RESIDENT.  Where the one-launch kernel does not cover a shape
(kc.RESIDENT_SHAPES says where it does) uis_stream_begin refuses UIS_FLAG_RESIDENT: the test asserts that refusal and
runs the shape on the path the library itself picks (flags 0).

  1. chunkings: one frame, three frames, ragged with silent slots, whole -- each the reference and the offline decode
  2. no table and an all-zero table: labels, scores and the exported bytes of the untagged session
  3. tag 127 at a slot's first frame            4. every cluster bound
  5. tags, a bias table and max_speakers together
  6. commits with and without a horizon between tagged pushes, every readout after every operation
  7. prime with tags: the continuation, the NLL, the contradiction refusal
  8. retire: the query omits tagged clusters, a list naming one is refused, the binding moves, the next tagged frames land
  9. export / import of a tagged utterance: another slot, another session, export(import(b)) == b, a persistent session
 10. restart: the slot's next utterance binds afresh, the neighbours' bytes are unchanged
 11. refusals: a persistent push with a table, a length mismatch, a tag of 128, a table pending across uis_stream_labels
 12. the one-frame chunking under UIS_POISON_WORKSPACE
"""

import numpy as np
import pytest

import known_session_cases as kc
import test_gpu_hostile as gh
from oracle import oracle
from uisrnn_amd import _capi

pytestmark = pytest.mark.gpu

PATHS = {'stepwise': _capi.UIS_FLAG_STEPWISE, 'resident': _capi.UIS_FLAG_RESIDENT}
WORDS = ('ffffffff', '7f7f7f7f', '80000000')   # test_gpu_poison.py's
KNOB = 'UIS_POISON_WORKSPACE'
ALL = [(name, path) for name in kc.SHAPES for path in PATHS]
MAIN = ALL
IDS = lambda cases: ['{}-{}'.format(*c) for c in cases]   # pylint: disable=unnecessary-lambda-assignment


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _refused(status, call):
  with pytest.raises(_capi.HipLibraryError) as err:
    call()
  assert err.value.status == status, err.value
  return str(err.value)


def _begin(dec, sh, path, limits=None):
  flags = PATHS[path]
  shape = dict(max_clusters=sh.cap, limits=limits)
  if path == 'resident' and sh.name not in kc.RESIDENT_SHAPES:
    _refused(_capi.UIS_ERR_UNSUPPORTED, lambda: dec.stream_begin(sh.n_utt, sh.beam, sh.window, flags=flags, **shape))
    flags = 0
  dec.stream_begin(sh.n_utt, sh.beam, sh.window, flags=flags, **shape)


def _check(dec, sh, snap, what, slots=None):
  """Every readout of the open session against the reference's snapshot (slots: {device slot: reference slot})."""
  lab, scores, overflow, status = dec.stream_labels()
  nb = dec.stream_nbest(sh.beam)
  bind = dec.stream_bindings()
  received, committed = dec.stream_received(), dec.stream_committed()
  assert status == _capi.UIS_OK and nb['status'] == _capi.UIS_OK, what
  for u, r in (slots or {u: u for u in range(sh.n_utt)}).items():
    col, n, at = snap[r], int(nb['counts'][u]), what + ('slot', u)
    assert n == col['live'] and not overflow[u], at
    assert nb['labels'][u][:n].tolist() == col['rows'], at
    assert _bits(nb['scores'][u][:n]).tolist() == col['scores'], at
    assert np.isinf(nb['scores'][u][n:]).all(), at
    if n:
      assert lab[u].tolist() == col['rows'][0] and int(_bits(scores[u:u + 1])[0]) == col['scores'][0], at
    assert bind[u].tolist() == col['bind'], at
    assert (int(received[u]), int(committed[u])) == (col['have'], col['committed']), at


def _apply(dec, sh, st, what):
  kind, call, want = st['kind'], st['call'], st['result']
  if kind in ('push', 'tag'):
    dec.stream_push(call['chunks'], bias=call['bias'], speakers=call['speakers'])
  elif kind == 'commit':
    labels, dropped = dec.stream_commit(call['horizons'])
    assert [x.tolist() for x in labels] == want['labels'] and dropped.tolist() == want['dropped'], what
  elif kind == 'query':
    got = dec.stream_retire(clusters=[None] * sh.n_utt)
    assert [x.tolist() for x in got['retirable']] == want['retirable'], what     # (tagged clusters are not listed)
    assert not any(len(x) for x in got['retired']), what
    bind = dec.stream_bindings()
    assert [sorted(int(k) for k in row[1:] if k >= 0) for row in bind] == [sorted(set(t)) for t in _rank0_tagged(st)], what
  elif kind == 'retire':
    got = dec.stream_retire(clusters=call['clusters'])
    assert [x.tolist() for x in got['retired']] == [c or [] for c in call['clusters']], what
  elif kind == 'restart':
    dec.stream_restart(call['which'])
  elif kind == 'prime':
    scores = dec.stream_prime(call['chunks'], call['labels'], speakers=call['speakers'])
    for u in range(sh.n_utt):
      assert int(_bits(scores)[u]) == want.get(u, 0), what + ('slot', u)
  else:
    raise ValueError(kind)


def _rank0_tagged(st):
  return [[k for k in col['bind'][1:] if k >= 0] for col in st['snap']]


def _replay(dec, name, plan, path, every=True, limits=None, between=None):
  """The trace of kc.PLANS[plan] on `dec`; every: all readouts after every operation (else after the last only).
  between(i, st): called before operation i with the session open."""
  sh, tr = kc.shape(name), kc.trace(name, plan)
  _begin(dec, sh, path, limits)
  try:
    for i, st in enumerate(tr):
      what = (name, plan, path, 'step', i, st['op'][0])
      if between:
        between(i, st)
      _apply(dec, sh, st, what)
      if every or i == len(tr) - 1:
        _check(dec, sh, st['snap'], what)
  finally:
    dec.stream_end()


def _run(name, plan, path, **more):
  dec = _capi.Decoder(kc.shape(name).params)
  try:
    _replay(dec, name, plan, path, **more)
  finally:
    dec.close()


# ---- 1. chunkings

@pytest.mark.parametrize('name,path', ALL, ids=IDS(ALL))
def test_every_chunking_is_the_reference_and_the_offline_decode(name, path, oracle_lib):
  sh = kc.shape(name)
  want = kc.trace(name, 'chunk_whole')[-1]['snap']
  lengths = kc.chunk_lengths(sh)
  seqs = [sh.pool[u][0][0][:n] for u, n in enumerate(lengths)]
  tags = [kc.life_tags(u, 0, kc.SEQ_LEN)[:n] for u, n in enumerate(lengths)]
  dec = _capi.Decoder(sh.params)
  try:
    for kind in kc.CHUNKINGS:
      _begin(dec, sh, path)
      try:
        got, silent = [0] * sh.n_utt, 0
        for chunks, flat in kc.chunk_calls(sh, kind):
          dec.stream_push(chunks, speakers=flat)
          got = [g + (0 if c is None else len(c)) for g, c in zip(got, chunks)]
          silent += sum(1 for u, c in enumerate(chunks) if c is None and got[u] < lengths[u])
        assert got == lengths and (kind != 'ragged' or silent), 'no slot was ever silent'
        _check(dec, sh, want, (name, path, kind))
      finally:
        dec.stream_end()
    # the offline decode of the same frames under the same tags
    frames, offsets = oracle.pack(seqs)
    out = dec.decode(frames, offsets, sh.beam, 1, 1, max_clusters=sh.cap, want_beam_scores=True, speakers=np.concatenate(tags))
    assert out['status'] == 0
    nb = dec.last_nbest(sh.beam)
    for u, col in enumerate(want):
      n = col['live']
      assert out['labels'][offsets[u]:offsets[u + 1]].tolist() == col['rows'][0], (name, path, 'offline', u)
      assert _bits(out['beam_scores'][u][:n]).tolist() == col['scores'] and int(nb['counts'][u]) == n
      assert nb['labels'][u][:n].tolist() == col['rows']
  finally:
    dec.close()


# ---- 2. no table, an all-zero table

def _first_difference(a, b):
  """Where two blobs differ, for an assertion's message: (offset, section) or None."""
  if a == b:
    return None
  at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
  f = _capi._BLOB_HEAD.unpack_from(a, 0)   # pylint: disable=protected-access
  beam, dp, hp, depth, n_window, live, n, lists = f[4], f[6], f[8], f[9], f[15], f[16], f[17], f[18]
  up = lambda x: (x + 15) & ~15   # pylint: disable=unnecessary-lambda-assignment
  ends, o = [('head', 96), ('ranks', 96 + 16 * live)], 96 + 16 * live
  for section, size in (('lists', 8 * lists), ('cnt', 4 * n)):
    o = up(o + size)
    ends.append((section, o))
  for section, size in (('mean', 4 * n * dp), ('hid', 4 * n * depth * hp)):
    o += size
    ends.append((section, o))
  ends.append(('records', up(o + 4 * n_window * beam)))
  return at, next((section for section, end in ends if at < end), 'trailer'), len(a), len(b)


@pytest.mark.parametrize('name,path', ALL, ids=IDS(ALL))
def test_an_all_zero_table_is_the_push_without_one(name, path, oracle_lib, monkeypatch):
  # (a blob carries the window's record words verbatim, those of ranks beyond a step's beam width included, which no
  # kernel ever writes: under the knob they hold the fill word in both sessions, and the bytes are the pushes' alone)
  monkeypatch.setenv(KNOB, WORDS[0])
  sh = kc.shape(name)
  dec = _capi.Decoder(sh.params)
  blobs = {}
  try:
    for plan in ('plain', 'zeros'):
      tr = kc.trace(name, plan)
      assert all((st['call']['speakers'] is None) == (plan == 'plain') for st in tr)
      assert plan == 'plain' or not any(st['call']['speakers'].any() for st in tr)
      _begin(dec, sh, path)
      try:
        for i, st in enumerate(tr):
          _apply(dec, sh, st, (name, plan, path, i))
        _check(dec, sh, tr[-1]['snap'], (name, plan, path))
        blobs[plan] = [dec.stream_export(u) for u in range(sh.n_utt)]
      finally:
        dec.stream_end()
    assert [_first_difference(a, b) for a, b in zip(blobs['plain'], blobs['zeros'])] == [None] * sh.n_utt
    assert all(_capi.blob_max_tag(b) == 0 for b in blobs['zeros'])
  finally:
    dec.close()


# ---- 3 - 7, 10. the plans

@pytest.mark.parametrize('plan', ['tag127', 'all_bound', 'together', 'commit', 'prime', 'restart'])
@pytest.mark.parametrize('name,path', MAIN, ids=IDS(MAIN))
def test_the_plans(name, path, plan, oracle_lib):
  sh = kc.shape(name)
  _run(name, plan, path, limits=list(kc.together_limits(sh)) if plan == 'together' else None)


@pytest.mark.parametrize('name,path', MAIN, ids=IDS(MAIN))
def test_a_prime_whose_labels_contradict_its_tags_is_refused(name, path, oracle_lib):
  sh = kc.shape(name)
  dec = _capi.Decoder(sh.params)
  _begin(dec, sh, path)
  try:
    dec.stream_push([sh.pool[0][0][0][:3]] + [None] * (sh.n_utt - 1), speakers=np.array([1, 0, 2], dtype=np.uint8))
    before = dec.stream_export(0)
    frames = [None, sh.pool[1][0][0][:3]] + [None] * (sh.n_utt - 2)
    for labels, tags in (([0, 1, 1], [3, 3, 0]), ([0, 0, 1], [3, 4, 0])):   # one tag on two labels; one label under two tags
      msg = _refused(_capi.UIS_ERR_INVALID_ARG, lambda: dec.stream_prime(  # pylint: disable=cell-var-from-loop
          frames, [None, np.array(labels, dtype=np.int32)] + [None] * (sh.n_utt - 2), speakers=np.array(tags, dtype=np.uint8)))  # pylint: disable=cell-var-from-loop
      assert 'the prefix labels contradict its tags' in msg
    assert dec.stream_export(0) == before and dec.stream_received().tolist() == [3] + [0] * (sh.n_utt - 1)
    assert dec.stream_bindings()[1].tolist() == [0] + [-1] * 127
    # the slot is as it was: the same prefix without the contradiction goes through
    dec.stream_prime(frames, [None, np.array([0, 1, 1], dtype=np.int32)] + [None] * (sh.n_utt - 2), speakers=np.array([3, 4, 0], dtype=np.uint8))
    row = dec.stream_bindings()[1]
    assert (row[0], row[3], row[4]) == (2, 0, 1)
  finally:
    dec.stream_end()
    dec.close()


# ---- 8. retire

@pytest.mark.parametrize('name,path', MAIN, ids=IDS(MAIN))
def test_retirement_keeps_tagged_clusters_and_moves_their_bindings(name, path, oracle_lib):
  sh = kc.shape(name)
  dec = _capi.Decoder(sh.params)

  def refuse_the_tagged_one(i, st):
    if st['kind'] != 'retire':
      return
    before = [dec.stream_export(u) for u in range(sh.n_utt)]
    # cluster 1 of slot 0 carries tag 5: naming it is the refusal of any cluster in use, and no bit changes
    _refused(_capi.UIS_ERR_INVALID_ARG, lambda: dec.stream_retire(clusters=[[1]] + [None] * (sh.n_utt - 1)))
    _refused(_capi.UIS_ERR_INVALID_ARG, lambda: dec.stream_retire(clusters=[[0, 1]] + [None] * (sh.n_utt - 1)))
    assert [dec.stream_export(u) for u in range(sh.n_utt)] == before
    assert dec.stream_bindings()[0][5] == 1

  try:
    _replay(dec, name, 'retire', path, between=refuse_the_tagged_one)
  finally:
    dec.close()


# ---- 9. export / import

@pytest.mark.parametrize('name,path', MAIN, ids=IDS(MAIN))
def test_a_tagged_utterance_moves_with_its_bindings(name, path, oracle_lib):
  sh = kc.shape(name)
  tr = kc.trace(name, 'chunk_three')
  want = tr[-1]['snap']
  src, dst = _capi.Decoder(sh.params), _capi.Decoder(sh.params)
  _begin(src, sh, path)
  _begin(dst, sh, path)
  try:
    for st in tr[:2]:
      _apply(src, sh, st, (name, path))
    blobs = [src.stream_export(u) for u in range(sh.n_utt)]
    assert any(_capi.blob_max_tag(b) > 0 for b in blobs), 'no blob carries a tag'
    _check(src, sh, tr[1]['snap'], (name, path, 'source'))
    # into another session, every stream one slot further; export(import(b)) == b
    turn = {(u + 1) % sh.n_utt: u for u in range(sh.n_utt)}
    for v, u in turn.items():
      dst.stream_import(v, blobs[u])
      assert dst.stream_export(v) == blobs[u], (name, path, v)
    _check(dst, sh, tr[1]['snap'], (name, path, 'arrived'), slots=turn)
    # into another slot of the same session: slot 1 ends, slot 0's stream continues there too
    src.stream_restart([u == 1 for u in range(sh.n_utt)])
    src.stream_import(1, blobs[0])
    assert src.stream_export(1) == blobs[0]
    twin = {u: (0 if u == 1 else u) for u in range(sh.n_utt)}
    for st in tr[2:]:
      call = st['call']
      sizes = [0 if c is None else len(c) for c in call['chunks']]
      at = np.concatenate([[0], np.cumsum(sizes)])
      parts = [call['speakers'][at[u]:at[u + 1]] for u in range(sh.n_utt)]
      src.stream_push([call['chunks'][twin[u]] for u in range(sh.n_utt)], speakers=np.concatenate([parts[twin[u]] for u in range(sh.n_utt)]))
      dst.stream_push([call['chunks'][turn[v]] for v in range(sh.n_utt)], speakers=np.concatenate([parts[turn[v]] for v in range(sh.n_utt)]))
    _check(src, sh, want, (name, path, 'twin'), slots=twin)
    _check(dst, sh, want, (name, path, 'moved'), slots=turn)
  finally:
    src.stream_end()
    dst.stream_end()
    src.close()
    dst.close()


def _persistent(dec, sh):
  if not gh._whole_device():   # pylint: disable=protected-access
    pytest.skip('not a whole MI355X')
  dec.stream_begin(sh.n_utt, sh.beam, sh.window, max_clusters=sh.cap, flags=_capi.UIS_FLAG_PERSISTENT)


def test_a_persistent_session_takes_no_tags(oracle_lib):
  """A push or a prime with a table and the import of a tagged blob: UIS_ERR_UNSUPPORTED, the table dropped, the slot as
  it was, the session usable."""
  name = 'one_launch'
  sh = kc.shape(name)
  tr = kc.trace(name, 'chunk_three')
  plain = kc.trace(name, 'plain')
  src, dec = _capi.Decoder(sh.params), _capi.Decoder(sh.params)
  _begin(src, sh, 'resident')
  try:
    for st in tr[:2]:
      _apply(src, sh, st, (name,))
    blob = src.stream_export(0)
    assert _capi.blob_max_tag(blob) > 0
  finally:
    src.stream_end()
    src.close()
  _persistent(dec, sh)
  try:
    call = tr[0]['call']
    assert 'dropped' in _refused(_capi.UIS_ERR_UNSUPPORTED, lambda: dec.stream_push(call['chunks'], speakers=call['speakers']))
    assert dec.stream_received().tolist() == [0] * sh.n_utt
    _refused(_capi.UIS_ERR_UNSUPPORTED, lambda: dec.stream_prime(
        [call['chunks'][0][:2]] + [None] * (sh.n_utt - 1), [np.zeros(2, dtype=np.int32)] + [None] * (sh.n_utt - 1),
        speakers=np.array([1, 1], dtype=np.uint8)))
    _refused(_capi.UIS_ERR_UNSUPPORTED, lambda: dec.stream_import(0, blob))
    assert dec.stream_received().tolist() == [0] * sh.n_utt
    for st in plain:   # the table was dropped: the pushes that follow are the untagged session's
      dec.stream_push(st['call']['chunks'])
    _check(dec, sh, plain[-1]['snap'], (name, 'persistent'))
  finally:
    dec.stream_end()
    dec.close()


# ---- 10. restart: the neighbours' bytes

@pytest.mark.parametrize('name,path', MAIN, ids=IDS(MAIN))
def test_a_restart_leaves_the_neighbours_bytes(name, path, oracle_lib):
  sh = kc.shape(name)
  dec = _capi.Decoder(sh.params)
  seen = {}

  def around(i, st):
    others = [u for u in range(sh.n_utt) if u != 1]
    if st['kind'] == 'restart':
      seen['before'] = [dec.stream_export(u) for u in others]
      assert dec.stream_bindings()[1][0] > 0
    elif 'before' in seen and 'after' not in seen:
      seen['after'] = [dec.stream_export(u) for u in others]
      assert dec.stream_bindings()[1].tolist() == [0] + [-1] * 127

  try:
    _replay(dec, name, 'restart', path, between=around)
    assert seen['before'] == seen['after']
  finally:
    dec.close()


# ---- 11. refusals

@pytest.mark.parametrize('name,path', MAIN, ids=IDS(MAIN))
def test_the_refusals_leave_the_session_as_it_was(name, path, oracle_lib):
  sh = kc.shape(name)
  tr = kc.trace(name, 'chunk_three')
  dec = _capi.Decoder(sh.params)
  _begin(dec, sh, path)
  try:
    _apply(dec, sh, tr[0], (name, path))
    before = [dec.stream_export(u) for u in range(sh.n_utt)]
    call = tr[1]['call']
    # a table of another length than the push's frames
    msg = _refused(_capi.UIS_ERR_INVALID_ARG, lambda: dec.stream_push(call['chunks'], speakers=call['speakers'][:-1]))
    assert 'uis_stream_speakers gave' in msg
    # a tag of 128: refused at uis_stream_speakers itself; nothing is pending afterwards
    _refused(_capi.UIS_ERR_INVALID_ARG, lambda: dec.set_stream_speakers(np.full(len(call['speakers']), 128)))
    assert [dec.stream_export(u) for u in range(sh.n_utt)] == before
    assert dec.stream_received().tolist() == [len(c) for c in tr[0]['call']['chunks']]
    # a table left pending survives the other session calls and reaches the next push
    dec.set_stream_speakers(call['speakers'])
    dec.stream_labels()
    dec.stream_nbest(1)
    dec.stream_bindings()
    dec.stream_retire(clusters=[None] * sh.n_utt)
    dec.stream_push(call['chunks'])
    _check(dec, sh, tr[1]['snap'], (name, path, 'pending'))
    for st in tr[2:]:
      _apply(dec, sh, st, (name, path))
    _check(dec, sh, tr[-1]['snap'], (name, path, 'end'))
  finally:
    dec.stream_end()
    dec.close()


# ---- 12. nothing stale

@pytest.mark.parametrize('word', WORDS)
def test_the_one_frame_chunking_on_poisoned_memory(word, oracle_lib, monkeypatch):
  monkeypatch.setenv(KNOB, word)
  for name, path in MAIN:
    sh = kc.shape(name)
    dec = _capi.Decoder(sh.params)
    _begin(dec, sh, path)
    try:
      for chunks, flat in kc.chunk_calls(sh, 'one'):
        dec.stream_push(chunks, speakers=flat)
      _check(dec, sh, kc.trace(name, 'chunk_whole')[-1]['snap'], (name, path, word))
    finally:
      dec.stream_end()
      dec.close()
