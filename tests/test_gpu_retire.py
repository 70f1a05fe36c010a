"""Speaker retirement on the GPU (uis_stream_retire) against tests/retire_ref.py.

Every comparison is exact -- integer labels and ids, float32 bit patterns -- except the posteriors, which keep their
own bound (posterior_ref.tolerance).  A device session and one retire_ref.Session per utterance are driven in
lock-step and every readout is compared after every operation: labels and scores of every live hypothesis, the
stable frames, committed, the window's frame count, the largest K and the retirable set.  The model is the
closed-form tracker of tests/golden (tracker_d64_h300) on frames around distinct centroids, so that the reference
opens a cluster per speaker; every test first asserts on the reference alone that its scenario is real.
  1. a query changes nothing                       5. a persistent session
  2. four kinds of utterance in one call           6. stale memory
  3. explicit subsets and every refusal            7. neighbours, restart, prime
  4. survival past the cluster cap
(8, the random walk, is tests/test_gpu_retire_walk.py.)
"""

import ctypes
import functools

import numpy as np
import pytest

import golden_util
import posterior_ref
import primed_ref
import retire_ref
import test_gpu_hostile as gh
import uisrnn_amd
from oracle import oracle
from uisrnn_amd import _capi

pytestmark = pytest.mark.gpu

MODEL = 'tracker_d64_h300'
TEMPERATURE = 16.0
KNOB = 'UIS_POISON_WORKSPACE'
THREADS = 256   # UIS_RETIRE_THREADS of uisrnn_amd/csrc/uis_retire.hip
EXACT = ('labels', 'scores', 'beam', 'overflow', 'rows', 'nb_scores', 'counts', 'stable', 'committed', 'have', 'K',
         'retirable')


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _model(name=MODEL):
  oracle.lib()
  return primed_ref.Model(golden_util.load_case(name)['params'])


def frames(seed, ids, dim=64, noise=0.05):
  """One frame per entry of ids around that speaker's unit centroid."""
  rng = np.random.default_rng(seed)
  cent = rng.standard_normal((max(ids) + 1, dim))
  cent /= np.linalg.norm(cent, axis=1, keepdims=True)
  return cent[np.array(ids)] + noise * rng.standard_normal((len(ids), dim))


class Dev:
  """An open session of a Decoder plus what OnlineSession keeps: the committed labels and the retired ids."""

  def __init__(self, n_utt, beam, window, cap, flags=0, model=MODEL):
    self.dec = _capi.Decoder(_model(model).params)
    self.dec.stream_begin(n_utt, beam, window, max_clusters=cap, flags=flags)
    self.n, self.beam = n_utt, beam
    self.final = [[] for _ in range(n_utt)]
    self.gone = [[] for _ in range(n_utt)]

  def close(self):
    self.dec.stream_end()
    self.dec.close()

  def ids(self, u, local):
    return [retire_ref.to_global(int(v), self.gone[u]) for v in local]

  def push(self, chunks):
    self.dec.stream_push(chunks)

  def commit(self, horizons):
    out, dropped = self.dec.stream_commit(horizons)
    out = [self.ids(u, x) for u, x in enumerate(out)]
    for u in range(self.n):
      self.final[u].extend(out[u])
    return out, dropped.tolist()

  def retire(self, which=None, clusters=None):
    """Returns (ids retired per utterance, K per utterance)."""
    res = self.dec.stream_retire(which, clusters)
    out = [self.ids(u, x) for u, x in enumerate(res['retired'])]
    for u in range(self.n):
      self.gone[u] = sorted(self.gone[u] + out[u])
    return out, res['K'].tolist()

  def refused(self, clusters):
    """The status of a selection that must be refused."""
    with pytest.raises(_capi.HipLibraryError) as err:
      self.dec.stream_retire(clusters=clusters)
    return err.value.status

  def restart(self, which):
    labels, _, _, _ = self.dec.stream_restart([u in which for u in range(self.n)])
    out = {}
    for u in which:
      out[u] = self.final[u] + self.ids(u, labels[u])
      self.final[u], self.gone[u] = [], []
    return out

  def shot(self):
    """Every readout of every utterance, for the whole stream, in plain Python values; posteriors as arrays."""
    dec = self.dec
    lab, scores, overflow, _ = dec.stream_labels()
    info = np.empty((self.n, self.beam), dtype=np.float32)
    dec._check(dec._lib.uis_last_decode_info(dec._handle, None, info.ctypes.data_as(_capi._fp)), 'info')  # pylint: disable=protected-access
    nb = dec.stream_nbest(self.beam)
    post = dec.stream_posterior(TEMPERATURE)
    query = dec.stream_retire(clusters=[None] * self.n)
    assert all(len(r) == 0 for r in query['retired'])
    have, done = dec.stream_received(), dec.stream_committed()
    cols = []
    for u in range(self.n):
      cnt = int(nb['counts'][u])
      cols.append({
          'labels': self.final[u] + self.ids(u, lab[u]), 'scores': int(_bits(scores[u:u + 1])[0]),
          'beam': _bits(info[u]).tolist(), 'overflow': int(overflow[u]),
          'rows': [self.final[u] + self.ids(u, row) for row in nb['labels'][u][:cnt]],
          'nb_scores': _bits(nb['scores'][u]).tolist(), 'counts': cnt, 'stable': len(self.final[u]) + int(nb['stable'][u]),
          'committed': int(done[u]), 'have': int(have[u]), 'K': int(query['K'][u]),
          'retirable': self.ids(u, query['retirable'][u]),
          'post': (_bits(post['confidence'][u]).tolist(), _bits(post['change'][u]).tolist(),
                   _bits(post['weights'][u]).tolist(), int(post['counts'][u])),
          'post_values': (post['confidence'][u], post['change'][u], post['weights'][u][:int(post['counts'][u])]),
      })
    return cols


def plain(cols):
  """A snapshot without its array views: what `==` can compare."""
  return [{k: v for k, v in c.items() if k != 'post_values'} for c in cols]


def want(ref, beam):
  """The exact readouts of one utterance from its reference."""
  inf = _bits(np.full(beam, np.inf)).tolist()
  if ref.received == 0:
    col = {'labels': [], 'scores': 0, 'beam': inf, 'overflow': 0, 'rows': [], 'nb_scores': inf, 'counts': 0, 'stable': 0}
  elif not ref.beam:
    col = {'labels': list(ref.final) + [-1] * ref.have, 'scores': inf[0], 'beam': inf, 'overflow': 0, 'rows': [],
           'nb_scores': inf, 'counts': 0, 'stable': ref.committed}
  else:
    padded = _bits(primed_ref.padded_beam(ref.scores(), beam)).tolist()
    col = {'labels': ref.labels(), 'scores': padded[0], 'beam': padded, 'overflow': 0, 'rows': ref.global_rows(),
           'nb_scores': padded, 'counts': len(ref.beam), 'stable': ref.committed + ref.stable()}
  col.update({'committed': ref.committed, 'have': ref.have, 'K': ref.K(),
              'retirable': [retire_ref.to_global(k, ref.gone) for k in ref.retirable()]})
  return col


def same(dev, refs, what):
  """The device's readouts are the references'.  Returns the snapshot."""
  cols = dev.shot()
  for u, (got, ref) in enumerate(zip(cols, refs)):
    exp = want(ref, dev.beam)
    for key in EXACT:
      assert got[key] == exp[key], (what, u, key, got[key], exp[key])
    conf, change, weights = got['post_values']
    if ref.live and ref.have:
      c_ref, ch_ref, w_ref = posterior_ref.posterior(ref.rows(), ref.scores(), TEMPERATURE)
      tol = posterior_ref.tolerance(ref.live)
      assert len(conf) == ref.have and len(weights) == ref.live, (what, u)
      worst = max(np.abs(conf - c_ref).max(), np.abs(change - ch_ref).max(), np.abs(weights - w_ref).max())
      assert worst <= tol, (what, u, worst, tol)
    elif ref.live:   # a window that a commit emptied: the one hypothesis, no frames
      assert len(conf) == 0 and weights.tolist() == [1.0], (what, u)
  return cols


def both_push(dev, refs, chunks, cap, what):
  dev.push(chunks)
  for ref, part in zip(refs, chunks):
    if part is not None:
      for t in range(len(part)):   # (frame by frame: the overflow word is sticky, no beam on the way may pass the cap)
        with np.errstate(all='ignore'):
          ref.push(part[t:t + 1])
        assert max([len(h.means) for h in ref.beam] or [0]) <= cap, (what, 'the reference passes the cap')
  return same(dev, refs, what)


def both_commit(dev, refs, horizons, what):
  got, dropped = dev.commit(horizons)
  exp = [ref.commit(None if h < 0 else h) for ref, h in zip(refs, horizons)]
  assert got == [e[0] for e in exp] and dropped == [e[1] for e in exp], (what, got, exp)
  return same(dev, refs, what)


def both_retire(dev, refs, which, what, clusters=None):
  """which: the utterances that retire everything retirable (None: all); clusters: explicit present indices instead."""
  if clusters is None:
    picks = [ref.retirable() if which is None or u in which else [] for u, ref in enumerate(refs)]
    got, k = dev.retire(None if which is None else [u in which for u in range(dev.n)])
  else:
    picks = [list(c or []) for c in clusters]
    got, k = dev.retire(clusters=clusters)
  exp = [ref.retire(p) for ref, p in zip(refs, picks)]
  assert got == exp and k == [ref.K() for ref in refs], (what, got, exp, k)
  return same(dev, refs, what)


# ---- 1, 2, 6: four kinds of utterance in one call

SPEAKERS = {
    'never': [0, 0, 1, 1, 1] + [0, 0, 0, 1, 1, 1] * 4,          # receives frames after the commit: never committed
    'old': [0, 0, 0, 1, 1, 2, 2] + [1, 1, 1, 2, 2, 2] * 4,      # speaker 0 is left behind by the commit
    'silent': [0, 0, 0, 1, 1, 1] * 4,                           # nothing until the retirement is over
    'emptied': [0, 0, 1, 1] + [0, 0, 0, 1, 1, 1] * 4,           # horizon 0 over an even window: nothing stays in it
}
FIRST = {'never': 5, 'old': 7, 'silent': 0, 'emptied': 4}
ORDER = ('never', 'old', 'silent', 'emptied')   # the utterance with retirable clusters is not the first: its records
                                                # start at window * beam words, unaligned where that is odd


def _four(beam, cap, window, check_query=False):
  model = _model()
  seqs = {k: frames(100 + i, SPEAKERS[k]) for i, k in enumerate(ORDER)}
  refs = [retire_ref.Session(model, beam) for _ in ORDER]
  dev = Dev(4, beam, window, cap)
  try:
    first = [seqs[k][:FIRST[k]] if k in ('old', 'emptied') else None for k in ORDER]
    both_push(dev, refs, first, cap, 'the first frames')
    both_commit(dev, refs, [-1, 3, -1, 0], 'the commit')
    both_push(dev, refs, [seqs['never'][:5], None, None, None], cap, 'the utterance that never commits')
    never, old, silent, emptied = refs
    # the scenario is real, on the reference alone
    assert old.committed > 0 and old.have > 0 and old.retirable(), 'nothing retirable after the commit'
    assert never.committed == 0 and never.have == 5 and never.K() >= 2 and never.retirable() == []
    assert silent.received == 0 and silent.retirable() == []
    assert emptied.have == 0 and emptied.committed == 4 and emptied.retirable() and emptied.beam[0].last > 0
    if beam > 1:
      assert (old.have * beam) % 4 != 0, 'the record words of the window are a multiple of four'
    if check_query:
      before = plain(same(dev, refs, 'before the query'))
      for call in (dict(clusters=[None] * 4), dict(clusters=[[], None, [], []]), dict(which=[0, 0, 0, 0])):
        res = dev.dec.stream_retire(**call)
        assert [len(r) for r in res['retired']] == [0] * 4 and res['K'].tolist() == [r.K() for r in refs], call
        assert [x.tolist() for x in res['retirable']] == [r.retirable() for r in refs], call
        assert plain(dev.shot()) == before, call   # to the bit
    both_retire(dev, refs, None, 'the retirement')
    assert old.retired[-1] and emptied.retired[-1] and not never.retired[-1] and not silent.retired[-1]
    pos = dict(FIRST, never=5)
    for i in range(12):   # 24 more frames in chunks of 1 and 3
      n = 1 if i % 2 == 0 else 3
      chunks = [seqs[k][pos[k]:pos[k] + n] for k in ORDER]
      for k in ORDER:
        pos[k] += n
      both_push(dev, refs, chunks, cap, ('push', i))
    assert old.received == 7 + 24 and all(r.beam for r in refs)
  finally:
    dev.close()


def test_a_query_changes_nothing(oracle_lib):
  _four(3, 8, 32, check_query=True)


@pytest.mark.parametrize('beam,cap,window', [(1, 4, 32), (3, 4, 33), (3, 8, 32), (10, 8, 33), (10, 8, 32), (1, THREADS + 44, 32)])
def test_four_kinds_of_utterance_in_one_call(beam, cap, window, oracle_lib):
  """beam 3 with window 33: the utterances' records are not 16-byte aligned (the scalar path); window 32: aligned, with
  a scalar tail; max_clusters 300 > the kernels' 256 threads at beam 1: every loop over Kmax takes a second turn."""
  _four(beam, cap, window)


@pytest.mark.parametrize('word', ('ffffffff', '7f7f7f7f'))
def test_no_output_depends_on_stale_memory(word, oracle_lib, monkeypatch):
  """Stale record words (ranks that are not live) go through the shift table: any bit pattern, the same results."""
  monkeypatch.setenv(KNOB, word)
  monkeypatch.delenv('UIS_NO_ARENA', raising=False)
  _four(3, 4, 33)


# ---- 3: explicit subsets and every refusal

def test_explicit_subsets_and_every_refusal(oracle_lib):
  beam, cap, window = 4, 16, 32
  model = _model()
  walk = retire_ref.speaker_walk(21, 64, 8, 2, 48)
  other = frames(104, SPEAKERS['old'])
  refs = [retire_ref.Session(model, beam) for _ in range(3)]
  # where to stop, from the reference alone: two retirable clusters, and one that only a hypothesis other than the best
  # one still uses in the window
  probe = retire_ref.Session(model, beam)
  stop = None
  for t in range(len(walk)):
    probe.push(walk[t:t + 1])
    if t % 2 == 1 and t >= 9:
      trial = retire_ref.Session(model, beam)
      trial.beam, trial.received, trial.committed, trial.final = list(probe.beam), probe.received, probe.committed, list(probe.final)
      trial.commit(5)
      rows = trial.rows()
      only_others = sorted(set(rows[1:].ravel().tolist()) - set(rows[0].tolist()) - {h.last for h in trial.beam})
      if len(trial.retirable()) >= 2 and len(trial.beam) > 1 and only_others:
        stop = t + 1
        break
  assert stop is not None, 'no frame count with two retirable clusters and a cluster only a lower hypothesis uses'
  dev = Dev(3, beam, window, cap)
  try:
    both_push(dev, refs, [walk[:stop], other[:7], None], cap, 'the first frames')
    both_commit(dev, refs, [5, 3, -1], 'the commit')
    ref = refs[0]
    able, rows = ref.retirable(), ref.rows()
    only_others = sorted(set(rows[1:].ravel().tolist()) - set(rows[0].tolist()) - {h.last for h in ref.beam})
    assert len(able) >= 2 and only_others and refs[1].retirable()
    good_other = refs[1].retirable()
    min_k = min(len(h.means) for h in ref.beam)
    assert min_k < cap
    before = plain(same(dev, refs, 'before the refusals'))
    refusals = {
        'used only by a hypothesis that is not the best': [[only_others[0]], None, None],
        'the last label': [[ref.beam[0].last], None, None],
        'not below every live K': [[min_k], None, None],
        'out of range': [[cap], None, None],
        'negative': [[-1], None, None],
        'a duplicate': [[able[0], able[0]], None, None],
        'a descending pair': [[able[1], able[0]], None, None],
        'bad for one utterance beside good ones': [[able[0]], [good_other[0], cap - 1] if cap - 1 not in good_other else [0, 0], None],
        'an utterance that has received nothing': [None, None, [0]],
    }
    for why, sel in refusals.items():
      assert dev.refused(sel) == _capi.UIS_ERR_INVALID_ARG, why
      assert plain(dev.shot()) == before, why   # the whole session, to the bit
    # every second retirable cluster of the first utterance, all of the second
    both_retire(dev, refs, None, 'an explicit subset', clusters=[able[::2], good_other, None])
    assert refs[0].retirable() == [k - sum(1 for r in able[::2] if r < k) for k in able[1::2]]
    for i in range(4):
      both_push(dev, refs, [walk[stop + 2 * i:stop + 2 * i + 2], other[7 + i:8 + i], other[i:i + 1]], cap, ('push', i))
    both_retire(dev, refs, None, 'the rest')
  finally:
    dev.close()


# ---- 4: survival

def _online(beam, cap, name=MODEL):
  params = _model(name).params
  model_args, _, args = uisrnn_amd.parse_arguments(
      ['--observation_dim', str(int(params['observation_dim'])), '--rnn_hidden_size', str(int(params['rnn_hidden_size']))])
  model = uisrnn_amd.UISRNN(model_args)
  model.load_params(params)
  args.beam_size, args.look_ahead, args.test_iteration, args.max_clusters = beam, 1, 1, cap
  return model, args


def test_a_session_survives_thirty_speakers_under_a_cap_of_six(oracle_lib):
  cap, beam, window, horizon, retire_at = 6, 4, 32, 8, 4
  seq = retire_ref.speaker_walk(11, 64, 30, 3, 90)
  # the control, on the reference alone: without retirement the best hypothesis passes the cap
  control = retire_ref.Session(_model(), beam)
  control.push(seq[:40])
  assert len(control.beam[0].means) > cap
  ref = retire_ref.AutoSession(_model(), beam, horizon, retire_at)
  model, args = _online(beam, cap)
  handed = {}   # id -> the stream position it was first handed out at
  with model.online(1, args, window, horizon=horizon, retire_at=retire_at) as session:
    pos = 0
    while pos < len(seq):
      n = 1 if pos % 3 else 2   # cap - retire_at = 2 is the longest chunk
      session.push([seq[pos:pos + n]])
      ref.push(seq[pos:pos + n])
      pos += n
      assert ref.most <= cap
      rows, scores = session.nbest()[0]
      assert rows == ref.global_rows() and _bits(scores).tolist() == _bits(ref.scores()).tolist(), pos
      assert session.labels()[0] == ref.labels() and session.committed == [ref.committed], pos   # (labels() raises on overflow)
      assert session.stable_frames() == [ref.committed + ref.stable()], pos
      assert session._gone[0] == ref.gone if session._gone else not ref.gone, pos   # pylint: disable=protected-access
      assert session.cluster_counts()[0] == (ref.K(), [retire_ref.to_global(k, ref.gone) for k in ref.retirable()]), pos
      for t, c in enumerate(ref.labels()):
        handed.setdefault(c, t)
    labels = session.labels()[0]
  assert len(ref.gone) >= 20 and max(labels) >= 29   # thirty speakers went by under a cap of six
  # ids are never reused: once retired an id does not come back, so every id's frames end before its retirement
  retired_at = {}
  for received, _, ids in ref.events:
    for c in ids:
      assert c not in retired_at
      retired_at[c] = received
  for c, at in retired_at.items():
    assert all(t < at for t, x in enumerate(labels) if x == c), c


# ---- 5: a persistent session

def test_retirement_between_the_pushes_of_a_persistent_session(oracle_lib):
  if not gh._whole_device():   # pylint: disable=protected-access
    pytest.skip('not a whole MI355X')
  name, beam, cap, window = 'tracker_d256', 2, 8, 32
  seq = frames(300, SPEAKERS['old'][:15], dim=256)
  ref = retire_ref.Session(_model(name), beam)
  ref.push(seq[:7])
  ref.commit(3)
  assert ref.retirable()
  shots = {}
  for flags in (_capi.UIS_FLAG_PERSISTENT, 0):
    try:
      dev = Dev(1, beam, window, cap, flags=flags, model=name)
    except _capi.HipLibraryError as err:
      if flags and err.status == _capi.UIS_ERR_UNSUPPORTED:
        pytest.skip('the session falls back to ordinary launches')
      raise
    try:
      out = []
      for t in range(7):
        dev.push([seq[t:t + 1]])
      out.append(dev.commit([3]))
      out.append(dev.retire())          # (the resident launch leaves for it: pm_quit)
      out.append(plain(dev.shot()))
      for t in range(7, 15):
        dev.push([seq[t:t + 1]])
      out.append(plain(dev.shot()))
      shots[flags] = out
    finally:
      dev.close()
  assert shots[_capi.UIS_FLAG_PERSISTENT] == shots[0]
  assert shots[0][1][0] == [ref.retire(ref.retirable())] and shots[0][1][0][0]
  ref.push(seq[7:15])
  assert shots[0][3][0]['rows'] == ref.global_rows() and shots[0][3][0]['nb_scores'][:len(ref.beam)] == _bits(ref.scores()).tolist()


# ---- 7: neighbours, restart, prime

def test_neighbours_restart_and_prime(oracle_lib):
  beam, cap = 4, 8
  seq = frames(104, SPEAKERS['old'])
  refs = [retire_ref.Session(_model(), beam) for _ in range(3)]
  model, args = _online(beam, cap)
  bad = seq[:3].copy()
  bad[2, 0] = np.inf
  with model.online(3, args, 32) as session:
    def check(what):
      got = session.nbest()
      for u, ref in enumerate(refs):
        if ref.live:
          assert got[u][0] == ref.global_rows() and _bits(got[u][1]).tolist() == _bits(ref.scores()).tolist(), (what, u)
        else:
          assert got[u] == ([], []), (what, u)
    session.push([seq[:7], seq[:7], bad])
    with np.errstate(all='ignore'):
      for ref, part in zip(refs, (seq[:7], seq[:7], bad)):
        ref.push(part)
    assert not refs[2].beam   # the non-finite frame emptied its beam
    got = session.commit([3, 3, 3])
    assert got == [ref.commit(3)[0] for ref in refs]
    assert refs[0].retirable() and refs[1].retirable()
    counts = session.cluster_counts()
    assert counts[2] == (0, []) and counts[1] == (refs[1].K(), refs[1].retirable())
    raw = session._decoder   # pylint: disable=protected-access
    before = (raw.stream_nbest(beam), raw.stream_posterior(TEMPERATURE))
    assert session.retire([0, 2]) == [refs[0].retire(refs[0].retirable()), [], []]   # the emptied beam reports nothing
    after = (raw.stream_nbest(beam), raw.stream_posterior(TEMPERATURE))
    for u in (1, 2):   # not selected, or dead: untouched to the bit
      assert np.array_equal(before[0]['labels'][u], after[0]['labels'][u]) and before[0]['counts'][u] == after[0]['counts'][u]
      assert _bits(before[0]['scores'][u]).tolist() == _bits(after[0]['scores'][u]).tolist()
      assert _bits(before[1]['confidence'][u]).tolist() == _bits(after[1]['confidence'][u]).tolist()
    assert session.cluster_counts()[1] == counts[1]
    check('after the retirement')
    session.push([seq[7:10], seq[7:10], None])
    refs[0].push(seq[7:10])
    refs[1].push(seq[7:10])
    check('three frames later')
    assert session.labels()[0] == refs[0].labels() and session._gone[0] == refs[0].gone   # pylint: disable=protected-access
    # restart: the result carries the stream's ids, the slot is fresh and its id map is cleared
    out = session.restart([0])
    assert out[0][0] == refs[0].labels() and session._gone[0] == [] and session.committed[0] == 0   # pylint: disable=protected-access
    prefix = [0, 0, 0, 1, 1]
    scores = session.prime([seq[:5], None, None], [prefix, None, None])
    start = primed_ref.advance_forced(_model(), seq[:5], prefix)
    refs[0] = retire_ref.Session(_model(), beam, start)
    assert _bits([scores[0]]).tolist() == _bits([start.score]).tolist()
    session.push([seq[5:9], None, None])
    refs[0].push(seq[5:9])
    check('the primed slot')
    assert session.labels()[0] == refs[0].labels() and session.cluster_counts()[0] == (refs[0].K(), [])
