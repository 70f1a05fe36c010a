"""No output may depend on stale memory: every API call under UIS_POISON_WORKSPACE (uisrnn_amd/csrc/uis_poison.h),
and one handle through many lives without the knob.

With the knob set the library fills every byte of working memory a call is about to use -- the workspace arena,
the staging buffers, the readouts' and the trainer's scratch -- with one word before the call's first write.  Three
words: ffffffff (a NaN as a float, -1 as an int, the highest counter value), 7f7f7f7f (a finite 3.4e38, a large
positive int) and 80000000 (-0.0: a sum that assumed +0 changes its sign bit).  A read that was defined only because
fresh memory happened to be benign, or because an earlier decode of the same shape left the right thing behind,
changes an output under at least one of them.

Every comparison is bit for bit (NaNs as test_gpu_hostile._same treats them), against the CPU oracle, the replay
of tests/nbest_ref.py, tests/forced_ref.py, the host's evaluation function -- or, for the trainer and the
_calculate_score arrays, against the same call without the knob.  DESIGN.md section 14 lists every buffer, what
defines it and which case here reaches it.
"""

import functools

import numpy as np
import pytest

import forced_ref
import hostile
import nbest_ref
import test_gpu_hostile as gh
import test_gpu_nbest as gn
import test_gpu_train_edges as te
from oracle import oracle
from uisrnn_amd import _capi
from uisrnn_amd import evals
from uisrnn_amd import synth
from uisrnn_amd import weights

pytestmark = pytest.mark.gpu

WORDS = ('ffffffff', '7f7f7f7f', '80000000')
KNOB = 'UIS_POISON_WORKSPACE'
FAMILIES = gh.FAMILIES
_same = gh._same   # pylint: disable=protected-access
DEBUG = _capi.UIS_FLAG_DEBUG_SCORES
RS_FAMILIES = ('rs_fixed', 'rs_generic', 'rs_padded')


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _env(monkeypatch, word, arena=True):
  """The knob (None: unset) and the workspace layout for the calls that follow."""
  if word is None:
    monkeypatch.delenv(KNOB, raising=False)
  else:
    monkeypatch.setenv(KNOB, word)
  if arena:
    monkeypatch.delenv('UIS_NO_ARENA', raising=False)
  else:
    monkeypatch.setenv('UIS_NO_ARENA', '1')


# ---- the data: benign tracker utterances and the subnormal regime, one oracle decode each

@functools.lru_cache(maxsize=None)
def _benign(shape, lengths):
  """Tracker weights and clean speaker-turn utterances (natural weights where the tracker's construction does not
  apply: fewer hidden units than features)."""
  dim, hidden, depth = shape
  if hidden >= dim:
    params = synth.tracker_params(dim, hidden, depth, seed=140 + dim)
  else:
    params = weights.init_params(dim, hidden, depth, sigma2=0.1, transition_bias=0.2, crp_alpha=1.0, seed=140 + dim)
  seqs, _ = synth.make_utterances(140_000 + 7 * dim, len(lengths), list(lengths), dim)
  return params, seqs


@functools.lru_cache(maxsize=None)
def _data(kind, shape, lengths, beam, look):
  """(params, seqs, the oracle's decode at test_iteration 1), shared by every case on the same data."""
  oracle.lib()
  if kind == 'benign':
    params, seqs = _benign(shape, lengths)
    return params, seqs, oracle.decode(params, seqs, beam, look, 1, n_threads=8)
  case = gh._case(kind, shape, lengths, 0)   # pylint: disable=protected-access
  return case.params, case.seqs, gh._reference(kind, shape, lengths, 0, beam, look)   # pylint: disable=protected-access


def _check_decode(out, ref, offsets, what, want=None, kind=None, seen=None):
  assert out['status'] == 0 and not out['overflow'].any(), what
  if want is not None:
    assert out['stats']['decode_kernel'].startswith(want), (what, out['stats']['decode_kernel'])
  if kind is not None:
    assert (out['stats']['decode_kernel_code'] >> 16) & 0xff == kind, (what, hex(out['stats']['decode_kernel_code']))
  for u in range(len(offsets) - 1):
    assert np.array_equal(out['labels'][offsets[u]:offsets[u + 1]], ref['labels'][u]), '%s: labels differ, utterance %d' % (what, u)
  _same(out['scores'], ref['scores'], what + ': scores')
  _same(out['beam_scores'], ref['beam_scores'], what + ': final beam')
  if seen is not None:
    assert out['stats']['max_clusters_seen'] == seen, what


# ---- every decode family

_FAMILY_CASES = [(fam, kind, arena) for fam in FAMILIES for kind in ('benign', 'subnormal')
                 for arena in ((True, False) if fam in RS_FAMILIES else (True,))]


@pytest.mark.parametrize('family,kind,arena', _FAMILY_CASES,
                         ids=['{}-{}-{}'.format(f, k, 'arena' if a else 'no_arena') for f, k, a in _FAMILY_CASES])
def test_every_decode_family(family, kind, arena, oracle_lib, monkeypatch):
  """The FAMILIES table of test_gpu_hostile.py at its shapes, each poison word in turn on one handle: labels, scores,
  the whole final beam, overflow, max_clusters_seen and the kernel's name against the oracle."""
  spec = FAMILIES[family]
  if spec.get('whole_device') and not gh._whole_device():   # pylint: disable=protected-access
    pytest.skip('not a whole MI355X')
  look = spec.get('look', 1)
  params, seqs, ref = _data(kind, spec['shape'], spec['lengths'], spec['beam'], look)
  seen = max(int(ref['max_clusters'].max()), 1)
  cap = spec.get('cap') or max(seen + look, 4)
  assert seen < cap, 'the case itself would hit the cluster cap'
  frames, offsets = oracle_lib.pack(seqs)
  _env(monkeypatch, None, arena)
  dec = _capi.Decoder(params)
  try:
    for word in WORDS:
      _env(monkeypatch, word, arena)
      out = dec.decode(frames, offsets, spec['beam'], look, 1, max_clusters=cap, flags=spec.get('flags', 0),
                       want_beam_scores=True)
      _check_decode(out, ref, offsets, '{} under {}'.format(family, word), spec['want'], spec.get('kind'), seen)
  finally:
    dec.close()


@pytest.mark.parametrize('kind', ['benign', 'subnormal'])
@pytest.mark.parametrize('family', ['rs_fixed', 'big_win'])
def test_calculate_score_arrays(family, kind, oracle_lib, monkeypatch):
  """UIS_FLAG_DEBUG_SCORES: every candidate score of every window has the unpoisoned run's bits (the array is +inf
  where _calculate_score pads; the decode's own outputs are the oracle's either way)."""
  spec = FAMILIES[family]
  look = spec.get('look', 1)
  params, seqs, ref = _data(kind, spec['shape'], spec['lengths'], spec['beam'], look)
  cap = spec.get('cap') or max(int(ref['max_clusters'].max()) + look, 4)
  frames, offsets = oracle_lib.pack(seqs)
  n_win = (max(spec['lengths']) + look - 1) // look
  _env(monkeypatch, None)
  dec = _capi.Decoder(params)
  try:
    runs = {}
    for word in (None,) + WORDS:
      _env(monkeypatch, word)
      out = dec.decode(frames, offsets, spec['beam'], look, 1, max_clusters=cap, flags=spec.get('flags', 0) | DEBUG,
                       want_beam_scores=True)
      _check_decode(out, ref, offsets, '{} with debug scores under {}'.format(family, word))
      runs[word] = (out['stats']['decode_kernel'], dec.debug_scores(n_win, len(seqs), spec['beam'], cap, look))
    assert np.isfinite(runs[None][1]).any() and np.isposinf(runs[None][1]).any()
    for word in WORDS:
      assert runs[word][0] == runs[None][0], word
      _same(runs[word][1], runs[None][1], '_calculate_score arrays under ' + word)
  finally:
    dec.close()


# ---- a decode in two launches: `resume` must survive, everything else may be poison

_SPLIT_UNIFORM = (150,) * 16
_SPLIT_RAGGED = (150, 143, 40, 129, 150, 136, 77, 78, 122, 150, 131, 149, 128, 76, 150, 145)


@functools.lru_cache(maxsize=None)
def _split_data(lengths):
  params = synth.tracker_params(256, 512, 1, seed=74)
  seqs, _ = synth.make_utterances(74_000, len(lengths), list(lengths), 256)
  oracle.lib()
  return params, seqs, oracle.decode(params, seqs, 10, 1, 1, n_threads=8)


@pytest.mark.parametrize('ragged', [False, True], ids=['uniform', 'ragged_f64'])
def test_two_launches_at_an_odd_boundary(ragged, oracle_lib, monkeypatch):
  """UIS_SPLIT_FRAMES=77 as in test_gpu_rs_args.py: a uniform float32 list and a ragged float64 list (staging block,
  scatter tables, utterances that end before, at and just behind the boundary)."""
  params, seqs, ref = _split_data(_SPLIT_RAGGED if ragged else _SPLIT_UNIFORM)
  frames, offsets = oracle_lib.pack(seqs)
  monkeypatch.setenv('UIS_SPLIT_MIN_MB', '0')
  monkeypatch.setenv('UIS_SPLIT_FRAMES', '77')
  _env(monkeypatch, None)
  dec = _capi.Decoder(params)
  try:
    for word in WORDS:
      _env(monkeypatch, word)
      if ragged:
        out = dec.decode_f64(seqs, 10, 1, 1, max_clusters=16, want_beam_scores=True)
      else:
        out = dec.decode(frames, offsets, 10, 1, 1, max_clusters=16, want_beam_scores=True)
      assert out['stats']['decode_launches'] == 2, (word, out['stats']['decode_launches'])
      _check_decode(out, ref, offsets, 'two launches under ' + word, 'k_decode_rs', gh.RS_FIXED)
  finally:
    dec.close()


# ---- n-best after a poisoned decode

@pytest.mark.parametrize('name,beam,look', [('tracker_d256', 10, 1), ('tiny_d16', 3, 1), ('d32_lookahead3', 4, 3)])
def test_every_rank_after_a_poisoned_decode(name, beam, look, oracle_lib, monkeypatch):
  """n_best = beam: every rank is walked from the final beam down to the first step, through the early steps whose
  beams were narrower than beam_size -- the ranks nobody wrote there hold the poison word and are clamped."""
  case = gn._case(name)   # pylint: disable=protected-access
  seqs = case['seqs']
  refs = [nbest_ref.nbest(gn._replay((name, u), case['params'], s, beam, look, 1)) for u, s in enumerate(seqs)]   # pylint: disable=protected-access
  if look == 1:   # (a first window of three frames already fills a beam of 4)
    assert any(len(gn._replay((name, u), case['params'], s, beam, look, 1).parents[0]) < beam   # pylint: disable=protected-access
               for u, s in enumerate(seqs)), 'no step narrower than the beam'
  _env(monkeypatch, None)
  dec = _capi.Decoder(case['params'])
  try:
    for word in WORDS:
      _env(monkeypatch, word)
      out, _, offsets = gn._decode(dec, seqs, beam, look, 1)   # pylint: disable=protected-access
      assert out['status'] == 0 and not out['overflow'].any(), word
      gn._compare(out, offsets, dec.last_nbest(beam), refs, beam)   # pylint: disable=protected-access
      gn._compare(out, offsets, dec.last_nbest(1), refs, 1)   # pylint: disable=protected-access
  finally:
    dec.close()


def test_an_utterance_at_the_cluster_cap_in_a_look_ahead_decode(oracle_lib, monkeypatch):
  """max_clusters 2 at look_ahead 2: a flagged utterance stops where it overflowed, the records of its later windows
  are poison; it counts 0 and reads -1, the others read what the unpoisoned decode gave them."""
  case = gn._case('tracker_d256')   # pylint: disable=protected-access
  seqs = [s[:24] for s in case['seqs']] + [case['seqs'][0][:2]]
  _env(monkeypatch, None)
  dec = _capi.Decoder(case['params'])
  try:
    out0, _, offsets = gn._decode(dec, seqs, 10, 2, 1, max_clusters=2)   # pylint: disable=protected-access
    assert out0['status'] == _capi.UIS_ERR_CLUSTER_CAP and out0['overflow'].any() and not out0['overflow'].all()
    want = dec.last_nbest(10)
    for word in WORDS:
      _env(monkeypatch, word)
      out, _, _ = gn._decode(dec, seqs, 10, 2, 1, max_clusters=2)   # pylint: disable=protected-access
      assert out['status'] == _capi.UIS_ERR_CLUSTER_CAP and np.array_equal(out['overflow'], out0['overflow']), word
      got = dec.last_nbest(10)
      for u in range(len(seqs)):
        if out['overflow'][u]:
          assert got['counts'][u] == 0 and np.all(got['labels'][u] == -1), (word, u)
        else:
          assert got['counts'][u] == want['counts'][u] > 0 and np.array_equal(got['labels'][u], want['labels'][u]), (word, u)
          assert np.array_equal(got['labels'][u][0], out['labels'][offsets[u]:offsets[u + 1]]), (word, u)
      _same(got['scores'], want['scores'], 'n-best scores under ' + word)
  finally:
    dec.close()


# ---- score_labels

@pytest.mark.parametrize('family', ['rs_fixed', 'small_h17_depth2'])
def test_score_labels(family, oracle_lib, monkeypatch):
  """Totals and per-frame losses of the oracle's labels and of an alternating labeling: forced_ref.score's bits."""
  spec = FAMILIES[family]
  params, seqs, ref = _data('subnormal', spec['shape'], spec['lengths'], spec['beam'], 1)
  case = gh._case('subnormal', spec['shape'], spec['lengths'], 0)   # pylint: disable=protected-access
  frames, offsets = oracle_lib.pack(seqs)
  wants = {name: forced_ref.score(params, seqs, labels) for name, labels in hostile.labelings(case, ref).items()}
  _env(monkeypatch, None)
  dec = _capi.Decoder(params)
  try:
    for word in WORDS:
      _env(monkeypatch, word)
      for name, labels in hostile.labelings(case, ref).items():
        scores, losses = dec.score_labels(frames, offsets, np.concatenate(labels), want_frame_losses=True)
        _same(scores, wants[name][0], '{} under {}: totals'.format(name, word))
        _same(losses, np.concatenate(wants[name][1]), '{} under {}: per-frame losses'.format(name, word))
  finally:
    dec.close()


# ---- sessions

def _best_after(rep, n):
  """The best hypothesis' labels after the first n frames (look_ahead 1, test_iteration 1)."""
  labels = np.empty(n, dtype=np.int32)
  r = 0
  for w in range(n - 1, -1, -1):
    labels[w] = rep.paths[w][r][0]
    r = int(rep.parents[w][r])
  return labels


@functools.lru_cache(maxsize=None)
def _session_data(n_utt):
  if n_utt == 64:   # the shape of test_persistent_launch_rows_that_change_hands_between_pushes, shorter utterances
    params = synth.tracker_params(256, 512, 1, seed=33)
    lens = [int(x) for x in np.random.default_rng(7).integers(12, 33, size=64)]
    seqs, _ = synth.make_utterances(12_700, len(lens), lens, 256)
  else:
    params = synth.tracker_params(256, 512, 1, seed=21)
    lens = [33, 1, 45, 17]
    seqs, _ = synth.make_utterances(12_000, len(lens), lens, 256)
  oracle.lib()
  ref = oracle.decode(params, seqs, 10, 1, 1, n_threads=8)
  reps = [nbest_ref.replay(params, s, 10, 1, 1) for s in seqs]
  for u, rep in enumerate(reps):   # (the replay and the oracle's decode agree: one reference)
    assert np.array_equal(_best_after(rep, len(seqs[u])), ref['labels'][u]), u
  return params, seqs, ref, reps


def _schedule(lens, chunk, seed):
  """Per-push frame counts: ragged pushes of 0 .. 16 frames (chunk None), else `chunk` frames each."""
  rng = np.random.default_rng(seed)
  left, schedule = list(lens), []
  while any(left):
    if chunk is None:
      top = int(rng.choice([1, 5, 16]))
      counts = [int(min(n, rng.integers(0, top + 1))) for n in left]
    else:
      counts = [min(n, chunk) for n in left]
    left = [n - c for n, c in zip(left, counts)]
    if any(counts):
      schedule.append(counts)
  return schedule


def _run_session(dec, seqs, ref, reps, schedule, flags, nbest_every, what):
  """One session: labels after every push, stream_nbest / stable every `nbest_every` pushes and at the end against
  the replay; final scores and the final beam against the oracle's offline decode."""
  dec.stream_begin(len(seqs), 10, max(len(s) for s in seqs), max_clusters=16, flags=flags)
  try:
    pos = [0] * len(seqs)
    for k, counts in enumerate(schedule):
      chunks = []
      for u, n in enumerate(counts):
        chunks.append(np.asarray(seqs[u][pos[u]:pos[u] + n], dtype=np.float32) if n else None)
        pos[u] += n
      dec.stream_push(chunks)
      labels, scores, overflow, status = dec.stream_labels()
      assert status == 0 and not overflow.any(), (what, k)
      for u in range(len(seqs)):
        assert np.array_equal(labels[u], _best_after(reps[u], pos[u])), (what, k, u)
      if (k + 1) % nbest_every == 0 or k == len(schedule) - 1:
        refs = [nbest_ref.nbest(r, upto=n) for r, n in zip(reps, pos)]
        got = dec.stream_nbest(10)
        assert got['status'] == 0, (what, k)
        gn._compare(None, np.concatenate([[0], np.cumsum(pos)]), got, refs, 10)   # pylint: disable=protected-access
        assert got['stable'].tolist() == [nbest_ref.common_prefix(rows) for rows, _ in refs], (what, k)
    assert pos == [len(s) for s in seqs]
    beam = np.empty((len(seqs), 10), dtype=np.float32)
    dec._check(dec._lib.uis_last_decode_info(dec._handle, None, beam.ctypes.data_as(_capi._fp)), 'info')   # pylint: disable=protected-access
  finally:
    dec.stream_end()
  _same(scores, ref['scores'], what + ': scores')
  _same(beam, ref['beam_scores'], what + ': final beam')


@pytest.mark.parametrize('persistent', [False, True], ids=['plain', 'persistent'])
@pytest.mark.parametrize('n_utt,chunk', [(64, None), (4, 1), (4, 7)], ids=['64_ragged', '4_by_1', '4_by_7'])
def test_sessions(n_utt, chunk, persistent, oracle_lib, monkeypatch):
  params, seqs, ref, reps = _session_data(n_utt)
  schedule = _schedule([len(s) for s in seqs], chunk, 7)
  _env(monkeypatch, None)
  dec = _capi.Decoder(params)
  try:
    for word in WORDS:
      _env(monkeypatch, word)
      _run_session(dec, seqs, ref, reps, schedule, _capi.UIS_FLAG_PERSISTENT if persistent else 0,
                   4 if n_utt == 64 else (8 if chunk == 1 else 1), 'session under ' + word)
  finally:
    dec.close()


# ---- evaluation

def _eval_pairs():
  """The random pairs of test_gpu_eval.py::test_random_pairs_against_the_host_function."""
  rng = np.random.default_rng(11)
  seqs1, seqs2 = [], []
  for trial in range(120):
    n = int(rng.integers(1, 700))
    k1 = int(rng.integers(1, 65 if trial % 7 == 0 else 9))
    k2 = int(rng.integers(1, 65 if trial % 5 == 0 else 9))
    a = rng.integers(0, k1, size=n)
    perm = rng.permutation(max(k1, k2))
    b = np.where(rng.random(n) < rng.random(), perm[a] % k2, rng.integers(0, k2, size=n))
    if trial % 3 == 0:
      seqs1.append(['spk{}'.format(v) for v in a])
    else:
      seqs1.append((a * 37 + 5).tolist())
    seqs2.append(b.tolist())
  return seqs1, seqs2


def test_evaluation(oracle_lib, monkeypatch):
  """uis_eval_accuracy on the random pairs against the host function, and uis_eval_last_decode on the labels a
  poisoned decode left on the device."""
  seqs1, seqs2 = _eval_pairs()
  want = [evals.compute_sequence_match_accuracy(x, y) for x, y in zip(seqs1, seqs2)]
  spec = FAMILIES['rs_fixed']
  params, seqs, ref = _data('benign', spec['shape'], spec['lengths'], spec['beam'], 1)
  frames, offsets = oracle_lib.pack(seqs)
  truth = np.concatenate([np.arange(len(s)) % 3 for s in seqs]).astype(np.int32)
  _env(monkeypatch, None)
  dec = _capi.Decoder(params)
  try:
    for word in WORDS:
      _env(monkeypatch, word)
      assert evals.sequence_match_accuracies_device(dec, seqs1, seqs2) == want, word
      dec.decode(frames, offsets, spec['beam'], 1, 1, max_clusters=spec['cap'])
      matched = dec.eval_last_decode(truth, len(seqs))
      host = dec.eval_matched(np.concatenate(ref['labels']), truth, offsets)
      assert np.array_equal(matched, host), word
      assert matched.tolist() == [round(evals.compute_sequence_match_accuracy(truth[offsets[u]:offsets[u + 1]].tolist(),
                                                                              ref['labels'][u].tolist()) * len(seqs[u]))
                                  for u in range(len(seqs))], word
  finally:
    dec.close()


# ---- the trainer

def _train_steps(name, **opts):
  params, sub = te.make_case(name)
  return te.run_step(params, sub, te.batch_of(name), steps=3, learning_rate=1e-2, dropout_key=te.KEY, **opts)


@pytest.mark.parametrize('name,dropout', [('B', 0.0), ('E', 0.4)])
def test_trainer(name, dropout, monkeypatch):
  """Three steps with the workspace poisoned before each: the losses, every gradient and every parameter after every
  step have the bits of an unpoisoned trainer from the same start (the trainer is deterministic)."""
  _env(monkeypatch, None)
  want = _train_steps(name, dropout=dropout)
  assert all(np.all(np.isfinite(g)) and np.any(g != 0) for _, g, _ in want)
  for word in WORDS:
    _env(monkeypatch, word)
    got = _train_steps(name, dropout=dropout)
    for step, ((l0, g0, p0), (l1, g1, p1)) in enumerate(zip(want, got)):
      assert np.array_equal(_bits(l1), _bits(l0)), (word, step, l1, l0)
      assert np.array_equal(_bits(g1), _bits(g0)), (word, step)
      assert np.array_equal(_bits(p1), _bits(p0)), (word, step)


# ---- one handle, many lives: no knob, the product as shipped

def _lives_params(dim, hidden):
  if hidden >= dim:
    return synth.tracker_params(dim, hidden, 1, seed=141)
  return weights.init_params(dim, hidden, 1, sigma2=0.1, transition_bias=0.2, crp_alpha=1.0, seed=141)


@functools.lru_cache(maxsize=None)
def _lives(dim, hidden):
  """The sequence's data and references, computed once for both layouts."""
  oracle.lib()
  params = _lives_params(dim, hidden)
  fixed, win, wide = FAMILIES['rs_fixed'], FAMILIES['big_win'], FAMILIES['stepwise_beam40']
  d = {'params': params}
  d['fixed'], _ = synth.make_utterances(141_000, len(fixed['lengths']), list(fixed['lengths']), dim)
  d['huge'] = hostile._overflow(d['fixed'])   # pylint: disable=protected-access
  d['win'], _ = synth.make_utterances(141_100, len(win['lengths']), list(win['lengths']), dim)
  d['wide'], _ = synth.make_utterances(141_200, len(wide['lengths']), list(wide['lengths']), dim)
  d['nan'], _ = synth.make_utterances(141_300, 3, [20, 15, 10], dim)
  d['nan'][1][7, 3] = np.nan
  d['ref_fixed'] = oracle.decode(params, d['fixed'], fixed['beam'], 1, 1, n_threads=8)
  d['ref_huge'] = oracle.decode(params, d['huge'], fixed['beam'], 1, 1, n_threads=8)
  d['ref_win'] = oracle.decode(params, d['win'], win['beam'], 2, 1, n_threads=8)
  d['ref_wide'] = oracle.decode(params, d['wide'], wide['beam'], 1, 1, n_threads=8)
  d['ref_nan'] = oracle.decode(params, d['nan'], 10, 1, 2, n_threads=8)
  assert not np.all(np.isfinite(d['ref_huge']['beam_scores'])), 'the huge features leave no inf behind'
  assert (d['ref_nan']['labels'][1] == -1).all() and (d['ref_nan']['labels'][0] >= 0).all()
  d['reps'] = [nbest_ref.replay(params, s, fixed['beam'], 1, 1) for s in d['fixed']]
  labels = [np.where(l < 0, 0, l).astype(np.int32) for l in d['ref_fixed']['labels']]
  d['forced'] = (labels, forced_ref.score(params, d['fixed'], labels))
  return d


@pytest.mark.parametrize('arena', [True, False], ids=['arena', 'no_arena'])
@pytest.mark.parametrize('dim,hidden', [(256, 512), (16, 8)])
def test_one_handle_many_lives(dim, hidden, arena, oracle_lib, monkeypatch):
  """One Decoder through decodes of growing and shrinking layouts, leftovers with inf and NaN in them, the readouts
  and two sessions: every result is the oracle's, and the first shape decoded again gives the bits of the first time."""
  d = _lives(dim, hidden)
  fixed, win, wide = FAMILIES['rs_fixed'], FAMILIES['big_win'], FAMILIES['stepwise_beam40']
  _env(monkeypatch, None, arena)
  dec = _capi.Decoder(d['params'])

  def decode(seqs, ref, beam, look, tau, what, cap=0, flags=0):
    frames, offsets = oracle_lib.pack(seqs)
    cap = cap or max(int(ref['max_clusters'].max()) + look, 4)
    out = dec.decode(frames, offsets, beam, look, tau, max_clusters=cap, flags=flags, want_beam_scores=True)
    _check_decode(out, ref, offsets, what)
    return out, frames, offsets

  try:
    first, frames, offsets = decode(d['fixed'], d['ref_fixed'], fixed['beam'], 1, 1, 'first', cap=fixed['cap'])
    decode(d['huge'], d['ref_huge'], fixed['beam'], 1, 1, 'huge features', cap=fixed['cap'])
    decode(d['win'], d['ref_win'], win['beam'], 2, 1, 'look_ahead 2')
    out, _, _ = decode(d['wide'], d['ref_wide'], wide['beam'], 1, 1, 'launch per step, beam 40', flags=_capi.UIS_FLAG_STEPWISE)
    assert out['stats']['decode_kernel'].startswith('stepwise')
    out, _, _ = decode(d['nan'], d['ref_nan'], 10, 1, 2, 'a non-finite frame', cap=16)
    assert np.isinf(out['scores'][1])
    again, _, _ = decode(d['fixed'], d['ref_fixed'], fixed['beam'], 1, 1, 'second', cap=fixed['cap'])
    for key in ('labels', 'scores', 'beam_scores', 'overflow'):
      assert again[key].tobytes() == first[key].tobytes(), key
    assert again['stats']['decode_kernel'] == first['stats']['decode_kernel']
    labels, (want_scores, want_losses) = d['forced']
    scores, losses = dec.score_labels(frames, offsets, np.concatenate(labels), want_frame_losses=True)
    _same(scores, want_scores, 'score_labels: totals')
    _same(losses, np.concatenate(want_losses), 'score_labels: per-frame losses')
    gn._compare(again, offsets, dec.last_nbest(fixed['beam']), [nbest_ref.nbest(r) for r in d['reps']], fixed['beam'])   # pylint: disable=protected-access
    schedule = _schedule([len(s) for s in d['fixed']], 5, 0)
    _run_session(dec, d['fixed'], d['ref_fixed'], d['reps'], schedule, 0, 2, 'plain session')
    if dim == 256:
      _run_session(dec, d['fixed'], d['ref_fixed'], d['reps'], schedule, _capi.UIS_FLAG_PERSISTENT, 2, 'persistent session')
    else:   # (the persistent launch exists for the cluster kernels' shapes: the refusal is a life too)
      with pytest.raises(_capi.HipLibraryError) as info:
        dec.stream_begin(len(d['fixed']), 10, 16, max_clusters=16, flags=_capi.UIS_FLAG_PERSISTENT)
      assert info.value.status == _capi.UIS_ERR_UNSUPPORTED
    third, _, _ = decode(d['fixed'], d['ref_fixed'], fixed['beam'], 1, 1, 'third', cap=fixed['cap'])
    for key in ('labels', 'scores', 'beam_scores', 'overflow'):
      assert third[key].tobytes() == first[key].tobytes(), key
  finally:
    dec.close()
