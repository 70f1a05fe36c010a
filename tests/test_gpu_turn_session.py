"""Minimum turn length in streaming sessions (uis_session_min_turn, uis_session_turns) on the GPU against
tests/turn_session_ref.py, bit for bit: the n-best rows, the scores, the final beam, the turns, the blobs' words.

Shapes are tests/session_walk.py's; the plans and their traces on the CPU reference are tests/turn_session_cases.py's
(computed once, shared, never written to; tests/test_turn_session_host.py asserts what they are meant to reach: the rule
changes the labels, no beam empties but the one that is meant to, no cap is in reach).  A slot's value is
(0, 2, 3, 5)[u % 4]: ruled and unruled slots share every launch.  Paths: the one the library picks (flags 0),
UIS_FLAG_STEPWISE, UIS_FLAG_STEPWISE | UIS_FLAG_GENERIC_SELECT and UIS_FLAG_RESIDENT.  Where the one-launch kernel does
not cover a shape (tc.RESIDENT_SHAPES says where it does) uis_stream_begin refuses UIS_FLAG_RESIDENT: the test asserts
that refusal and stops there -- flags 0 is a path of its own.

  1. chunkings: one frame, three frames, ragged with silent slots, whole -- each the reference and the offline decode
  2. a table of zeros and ones: the exported bytes of the session without one, under UIS_POISON_WORKSPACE
  3. commits with horizons, one of which empties every window; the run survives
  4. retire: the query omits the cluster the hypothesis speaks in, the label is renumbered under its run
  5. prime: the trailing run, a short turn inside, predict_primed(min_turn=) under beam 1
  6. export / import between values    7. restart and the fresh-slot rule of the setter
  8. the rule with tags, max_speakers and a bias table, one slot's beam emptied
  9. a persistent session             10. the one-frame chunking under UIS_POISON_WORKSPACE
"""

import struct

import numpy as np
import pytest

import test_gpu_hostile as gh
import turn_session_cases as tc
import turn_session_ref as tsr
import uisrnn_amd
from oracle import oracle
from uisrnn_amd import _capi

pytestmark = pytest.mark.gpu

PATHS = {'default': 0, 'stepwise': _capi.UIS_FLAG_STEPWISE, 'generic': _capi.UIS_FLAG_STEPWISE | _capi.UIS_FLAG_GENERIC_SELECT,
         'resident': _capi.UIS_FLAG_RESIDENT}
WORDS = ('ffffffff', '7f7f7f7f', '80000000')   # test_gpu_poison.py's
KNOB = 'UIS_POISON_WORKSPACE'
ALL = [(name, path) for name in tc.SHAPES for path in PATHS]
# the plans beyond the chunkings: the launch-per-step kernels and the one-launch kernel (where the shape has one, else
# the library's own choice)
MAIN = [(name, path) for name in tc.SHAPES for path in ('stepwise', 'resident' if name in tc.RESIDENT_SHAPES else 'default')]
IDS = lambda cases: ['{}-{}'.format(*c) for c in cases]   # pylint: disable=unnecessary-lambda-assignment


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _refused(status, call):
  with pytest.raises(_capi.HipLibraryError) as err:
    call()
  assert err.value.status == status, err.value
  return str(err.value)


def _begin(dec, sh, path, limits=None):
  """False where uis_stream_begin refuses UIS_FLAG_RESIDENT for the shape (asserted)."""
  shape = dict(max_clusters=sh.cap, limits=limits)
  if path == 'resident' and sh.name not in tc.RESIDENT_SHAPES:
    _refused(_capi.UIS_ERR_UNSUPPORTED, lambda: dec.stream_begin(sh.n_utt, sh.beam, sh.window, flags=PATHS[path], **shape))
    return False
  dec.stream_begin(sh.n_utt, sh.beam, sh.window, flags=PATHS[path], **shape)
  return True


def _words(blob):
  """(label, run) of every live rank's last-label word of a blob (csrc/uis_blob.h)."""
  live = _capi.blob_info(blob)['live']
  out = []
  for r in range(live):
    w = struct.unpack_from('<i', blob, 96 + 16 * r + 4)[0]
    out.append([-1, 0] if w < 0 else [w & 0xffff, (w >> 16) & 0x7fff])
  return out


def _check(dec, sh, snap, what, slots=None):
  """Every readout of the open session against the reference's snapshot (slots: {device slot: reference slot})."""
  lab, scores, overflow, status = dec.stream_labels()
  nb = dec.stream_nbest(sh.beam)
  turns = dec.session_turns()
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
      assert _words(dec.stream_export(u)) == col['words'], at
    elif col['have']:
      assert (lab[u] == -1).all() and np.isinf(scores[u]), at      # an emptied beam, reported as ever
    assert turns[u].tolist() == col['turns'], at
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
    assert [x.tolist() for x in got['retirable']] == want['retirable'], what
    assert not any(len(x) for x in got['retired']), what
  elif kind == 'retire':
    got = dec.stream_retire(clusters=call['clusters'])
    assert [x.tolist() for x in got['retired']] == [c or [] for c in call['clusters']], what
  elif kind == 'restart':
    dec.stream_restart(call['which'])
  elif kind == 'prime':
    scores = dec.stream_prime(call['chunks'], call['labels'])
    for u in range(sh.n_utt):
      assert int(_bits(scores)[u]) == want.get(u, 0), what + ('slot', u)
  elif kind == 'setm':
    dec.session_set_min_turn(call['values'])
    assert dec.session_min_turn().tolist() == call['values'], what
  else:
    raise ValueError(kind)


def _replay(dec, name, plan, path, every=True, limits=None, between=None):
  """The trace of tc.PLANS[plan] on `dec`; every: all readouts after every operation (else after the last only).
  between(i, st): called before operation i with the session open."""
  sh, tr = tc.shape(name), tc.trace(name, plan)
  assert _begin(dec, sh, path, limits)
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
  dec = _capi.Decoder(tc.shape(name).params)
  try:
    _replay(dec, name, plan, path, **more)
  finally:
    dec.close()


# ---- 1. chunkings

@pytest.mark.parametrize('name,path', ALL, ids=IDS(ALL))
def test_every_chunking_is_the_reference_and_the_offline_decode(name, path, oracle_lib):
  sh = tc.shape(name)
  want = tc.trace(name, 'chunk_whole')[-1]['snap']
  lengths = tc.chunk_lengths(sh)
  values = tc.slot_values(sh.n_utt)
  seqs = [sh.pool[u][0][0][:n] for u, n in enumerate(lengths)]
  dec = _capi.Decoder(sh.params)
  try:
    for kind in tc.CHUNKINGS:
      if not _begin(dec, sh, path):
        return   # (the refusal is asserted; the shape's other paths are this test's other cases)
      try:
        dec.session_set_min_turn(values)
        got, silent = [0] * sh.n_utt, 0
        for chunks in tc.chunk_calls(sh, kind):
          dec.stream_push(chunks)
          inst = dec.last_instantiation()
          if path == 'resident':
            assert inst[0] == 'k_decode_resident' and inst[4] == 0, (name, kind, inst)
          elif path in ('stepwise', 'generic'):
            assert inst[0] == 'stepwise', (name, kind, inst)
          got = [g + (0 if c is None else len(c)) for g, c in zip(got, chunks)]
          silent += sum(1 for u, c in enumerate(chunks) if c is None and got[u] < lengths[u])
        assert got == lengths and (kind != 'ragged' or silent), 'no slot was ever silent'
        _check(dec, sh, want, (name, path, kind))
      finally:
        dec.stream_end()
    # the offline decode of the same frames under the same values
    frames, offsets = oracle.pack(seqs)
    out = dec.decode(frames, offsets, sh.beam, 1, 1, max_clusters=sh.cap, want_beam_scores=True, min_turn=values)
    assert out['status'] == 0
    nb = dec.last_nbest(sh.beam)
    for u, col in enumerate(want):
      n = col['live']
      assert out['labels'][offsets[u]:offsets[u + 1]].tolist() == col['rows'][0], (name, path, 'offline', u)
      assert _bits(out['beam_scores'][u][:n]).tolist() == col['scores'] and int(nb['counts'][u]) == n
      assert nb['labels'][u][:n].tolist() == col['rows']
  finally:
    dec.close()


# ---- 2. zeros and ones

@pytest.mark.parametrize('name,path', MAIN, ids=IDS(MAIN))
def test_a_table_of_zeros_and_ones_is_the_session_without_one(name, path, oracle_lib, monkeypatch):
  # (a blob carries the window's record words verbatim, those of ranks beyond a step's beam width included, which no
  # kernel ever writes: under the knob they hold the fill word in both sessions, and the bytes are the pushes' alone)
  monkeypatch.setenv(KNOB, WORDS[0])
  sh = tc.shape(name)
  dec = _capi.Decoder(sh.params)
  blobs = {}
  try:
    for plan in ('plain', 'zeros_ones'):
      tr = tc.trace(name, plan)
      assert (tr[0]['kind'] == 'setm') == (plan == 'zeros_ones')
      assert _begin(dec, sh, path)
      try:
        for i, st in enumerate(tr):
          _apply(dec, sh, st, (name, plan, path, i))
        _check(dec, sh, tr[-1]['snap'], (name, plan, path))
        blobs[plan] = [dec.stream_export(u) for u in range(sh.n_utt)]
      finally:
        dec.stream_end()
    assert blobs['plain'] == blobs['zeros_ones']
    assert all(run == 0 for b in blobs['zeros_ones'] for _, run in _words(b))
  finally:
    dec.close()


# ---- 3, 5, 7. the plans

@pytest.mark.parametrize('plan', ['commit', 'prime', 'restart'])
@pytest.mark.parametrize('name,path', MAIN, ids=IDS(MAIN))
def test_the_plans(name, path, plan, oracle_lib):
  _run(name, plan, path)


# ---- 4. retire

@pytest.mark.parametrize('name,path', MAIN, ids=IDS(MAIN))
def test_retirement_reads_the_label_and_keeps_the_run(name, path, oracle_lib):
  sh = tc.shape(name)
  dec = _capi.Decoder(sh.params)

  def refuse_the_one_in_use(i, st):
    if st['kind'] != 'retire':
      return
    before = [dec.stream_export(u) for u in range(sh.n_utt)]
    assert dec.session_turns()[0].tolist() == [2, 2]
    # cluster 2 of slot 0 is the one the hypothesis speaks in: naming it is refused, and no bit changes
    _refused(_capi.UIS_ERR_INVALID_ARG, lambda: dec.stream_retire(clusters=[[2]] + [None] * (sh.n_utt - 1)))
    _refused(_capi.UIS_ERR_INVALID_ARG, lambda: dec.stream_retire(clusters=[[0, 1, 2]] + [None] * (sh.n_utt - 1)))
    assert [dec.stream_export(u) for u in range(sh.n_utt)] == before

  try:
    _replay(dec, name, 'retire', path, between=refuse_the_one_in_use)
  finally:
    dec.close()


# ---- 5. prime: predict_primed under beam 1

@pytest.mark.parametrize('name', ['deep', 'one_launch'])
def test_under_beam_1_a_decode_primed_with_its_own_opening_continues_bit_for_bit(name, oracle_lib):
  sh = tc.shape(name)
  model_args, _, inference_args = uisrnn_amd.parse_arguments(
      ['--observation_dim', str(int(sh.params['observation_dim'])), '--rnn_hidden_size', str(int(sh.params['rnn_hidden_size'])),
       '--rnn_depth', str(int(sh.params['rnn_depth']))])
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(sh.params)
  inference_args.beam_size, inference_args.look_ahead, inference_args.test_iteration = 1, 1, 1
  seqs = [sh.pool[u][0][0][:sh.window].astype(np.float64) for u in range(sh.n_utt)]
  whole = model.predict(seqs, inference_args, min_turn=3)
  # each prefix ends one frame into a turn where the decode has a second turn (the rule then holds the primed hypothesis
  # for two more frames), else after three frames
  changes = [[t for t in range(1, len(w)) if w[t] != w[t - 1]] for w in whole]
  cut = [c[0] + 1 if c else 3 for c in changes]
  assert any(changes), 'no decode has a second turn'
  primed = model.predict_primed(seqs, [w[:p] for w, p in zip(whole, cut)], inference_args, min_turn=3)
  assert primed == whole


# ---- 6. export / import

@pytest.mark.parametrize('name,path', MAIN, ids=IDS(MAIN))
def test_an_utterance_moves_between_slots_of_different_values(name, path, oracle_lib):
  """Slot 2 (m = 3; here a second session gives every value its turn) after its first frames: into a slot of the same
  value (export(import(b)) == b, the stream continues bit for bit), into one without a rule (bare labels, and from there
  the session without a rule), from there into m = 3 (run 3), and from m = 5 into m = 3 (clamped).  A restart leaves
  the neighbours' bytes."""
  sh = tc.shape(name)
  n0, n1 = 5, 4
  seq = sh.pool[2][0][0]

  def ref(m):
    s = tsr.Session(sh.model, sh.beam, m=m)
    s.push(seq[:n0])
    return s

  src3, src5 = ref(3), ref(5)
  targets = {'same': tsr.Session(sh.model, sh.beam, m=3).imported(src3), 'bare': tsr.Session(sh.model, sh.beam, m=0).imported(src3),
             'clamped': tsr.Session(sh.model, sh.beam, m=3).imported(src5)}
  targets['loose'] = tsr.Session(sh.model, sh.beam, m=3).imported(targets['bare'])
  arrived = {k: tc.snap([s])[0] for k, s in targets.items()}
  for s in list(targets.values()) + [src3]:
    s.push(seq[n0:n0 + n1])
  after = {k: tc.snap([s])[0] for k, s in targets.items()}
  cont = tc.snap([src3])[0]

  a, b = _capi.Decoder(sh.params), _capi.Decoder(sh.params)
  assert _begin(a, sh, path) and _begin(b, sh, path)
  try:
    # session a: slot 0 under 3, slot 1 under 5, slot 2 without a rule; session b: slot 0 under 3, slot 1 without, slot 2 under 3
    a.session_set_min_turn(([3, 5, 0] + [0] * sh.n_utt)[:sh.n_utt])
    b.session_set_min_turn(([3, 0, 3] + [0] * sh.n_utt)[:sh.n_utt])
    a.stream_push([seq[:n0], seq[:n0]] + [None] * (sh.n_utt - 2))
    blob3, blob5 = a.stream_export(0), a.stream_export(1)
    assert _words(blob3) == tc.snap([ref(3)])[0]['words'] and _words(blob5) == tc.snap([ref(5)])[0]['words']
    b.stream_import(0, blob3)                         # the same value
    assert b.stream_export(0) == blob3
    b.stream_import(1, blob3)                         # into a slot without a rule: bare labels
    bare = b.stream_export(1)
    assert _words(bare) == arrived['bare']['words'] and all(run == 0 for _, run in _words(bare))
    b.stream_import(2, blob5)                         # from m = 5 into m = 3: clamped
    assert _words(b.stream_export(2)) == arrived['clamped']['words']
    a.stream_import(2, bare)                          # (a's slot 2 has no rule: the bare blob as it is)
    assert a.stream_export(2) == bare
    _check(b, sh, [arrived['same'], arrived['bare'], arrived['clamped']], (name, path, 'arrived'), slots={0: 0, 1: 1, 2: 2})
    # a restart of slot 1 leaves the neighbours' bytes; then the bare blob into it under m = 3: run 3
    around = [b.stream_export(0), b.stream_export(2)]
    b.stream_restart([u == 1 for u in range(sh.n_utt)])
    assert [b.stream_export(0), b.stream_export(2)] == around
    values = b.session_min_turn().tolist()
    values[1] = 3
    b.session_set_min_turn(values)
    b.stream_import(1, bare)
    loose = b.stream_export(1)
    assert _words(loose) == arrived['loose']['words'] and all(run == 3 for _, run in _words(loose))
    # every stream goes on with the same frames
    part = seq[n0:n0 + n1]
    b.stream_push([part, part, part] + [None] * (sh.n_utt - 3))
    a.stream_push([part, None, part] + [None] * (sh.n_utt - 3))
    _check(b, sh, [after['same'], after['loose'], after['clamped']], (name, path, 'moved'), slots={0: 0, 1: 1, 2: 2})
    _check(a, sh, [cont, None, after['bare']], (name, path, 'stayed'), slots={0: 0, 2: 2})
  finally:
    a.stream_end()
    b.stream_end()
    a.close()
    b.close()


# ---- 7. the setter's fresh-slot rule

@pytest.mark.parametrize('name,path', MAIN, ids=IDS(MAIN))
def test_the_setter_refuses_a_slot_that_has_received_frames(name, path, oracle_lib):
  sh = tc.shape(name)
  tr = tc.trace(name, 'restart')
  dec = _capi.Decoder(sh.params)
  assert _begin(dec, sh, path)
  try:
    for st in tr[:2]:
      _apply(dec, sh, st, (name, path))
    values = tr[0]['call']['values']
    before = [dec.stream_export(u) for u in range(sh.n_utt)]
    changed = list(values)
    changed[2] = 5
    for bad in (changed, [5] + values[1:], [v + 1 for v in values]):
      assert 'nothing was changed' in _refused(_capi.UIS_ERR_INVALID_ARG, lambda: dec.session_set_min_turn(bad))  # pylint: disable=cell-var-from-loop
    fresh_too = list(changed)
    _refused(_capi.UIS_ERR_INVALID_ARG, lambda: dec.session_set_min_turn([32768] + values[1:]))
    _refused(_capi.UIS_ERR_INVALID_ARG, lambda: dec.session_set_min_turn([-1] + values[1:]))
    assert dec.session_min_turn().tolist() == values and [dec.stream_export(u) for u in range(sh.n_utt)] == before
    dec.session_set_min_turn(values)                  # the same table is no change
    _apply(dec, sh, tr[2], (name, path))              # slot 2 restarts: it keeps its value, the run is gone
    assert dec.session_min_turn().tolist() == values and dec.session_turns()[2].tolist() == [-1, 0]
    # all or nothing: the change that is legal now does not go through beside one that is not
    _refused(_capi.UIS_ERR_INVALID_ARG, lambda: dec.session_set_min_turn([5] + fresh_too[1:]))
    assert dec.session_min_turn().tolist() == values
    dec.session_set_min_turn(fresh_too)               # ... and alone it is accepted
    assert dec.session_min_turn().tolist() == fresh_too
    # a pending uis_min_turn table is a decode's: the session calls refuse it, and the session stays usable
    dec.set_min_turn(values)
    _refused(_capi.UIS_ERR_UNSUPPORTED, dec.session_turns)
    dec.session_turns()
    # without an open session the three calls are refused on a live handle
    dec.stream_end()
    for call in (dec.session_turns, dec.session_min_turn, lambda: dec.session_set_min_turn(values)):
      assert 'no streaming session' in _refused(_capi.UIS_ERR_INVALID_ARG, call)
  finally:
    dec.stream_end()
    dec.close()


# ---- 8. the rule with tags, max_speakers and a bias table

@pytest.mark.parametrize('name,path', MAIN, ids=IDS(MAIN))
def test_the_rule_with_tags_a_speaker_bound_and_a_bias_table(name, path, oracle_lib):
  sh = tc.shape(name)
  tr = tc.trace(name, 'together')
  assert tr[2]['snap'][2]['live'] == 0 and tr[2]['snap'][2]['have'] == 2, 'slot 2 was to lose its beam'
  assert all(col['live'] > 0 for u, col in enumerate(tr[-1]['snap']) if u != 2)
  assert tr[-1]['snap'][2]['live'] == 0 and tr[-1]['snap'][2]['turns'] == [-1, 0]
  _run(name, 'together', path, limits=list(tc.together_limits(sh)))


# ---- 9. a persistent session

def test_a_persistent_session_honours_the_rule(oracle_lib):
  """Under m = 3 the bits of the non-persistent session, across a set_min_turn after a restart that makes the resident
  launch leave and come back."""
  if not gh._whole_device():   # pylint: disable=protected-access
    pytest.skip('not a whole MI355X')
  name = 'one_launch'
  sh = tc.shape(name)
  tr = tc.trace(name, 'restart')
  dec = _capi.Decoder(sh.params)
  dec.stream_begin(sh.n_utt, sh.beam, sh.window, max_clusters=sh.cap, flags=_capi.UIS_FLAG_PERSISTENT)
  try:
    for i, st in enumerate(tr):
      _apply(dec, sh, st, (name, 'persistent', i))
      _check(dec, sh, st['snap'], (name, 'persistent', i))
    assert dec.last_instantiation()[4] == 1, 'no push ran on the persistent launch'
  finally:
    dec.stream_end()
    dec.close()


# ---- 10. nothing stale

@pytest.mark.parametrize('word', WORDS)
def test_the_one_frame_chunking_on_poisoned_memory(word, oracle_lib, monkeypatch):
  monkeypatch.setenv(KNOB, word)
  for name, path in MAIN:
    sh = tc.shape(name)
    dec = _capi.Decoder(sh.params)
    assert _begin(dec, sh, path)
    try:
      dec.session_set_min_turn([tc.M] * sh.n_utt)
      for chunks in tc.chunk_calls(sh, 'one'):
        dec.stream_push(chunks)
      _check(dec, sh, tc.trace(name, 'all3')[-1]['snap'], (name, path, word))
    finally:
      dec.stream_end()
      dec.close()
