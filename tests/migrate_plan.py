"""Plans for the export / import tests and their trace on the CPU reference.  No device, no library.

A stream's reference is tests/retire_ref.py's Session (commit_ref.Session with retirement; primed_ref.advance_forced
for a primed start): it does not know which slot it sits in, so moving an utterance means holding another slot to the
same reference object.  A PLAN is a list of concrete operations on one stream, laid out here with the reference at
hand so that the cut states are real:

  ('push', pos, n)       the stream's n frames from pos on (1 .. 5 of them)
  ('commit', h)          uis_stream_commit with horizon h for this stream (negative: none)
  ('retire',)            everything retirable
  ('prime', n, labels)   the first n frames as a labeled prefix
  ('cut', name)          a state in which the utterance is exported

A Trace holds, for every operation, what it must answer (`results`) and every readout of the stream afterwards
(`wants`: test_gpu_retire.want's column -- labels, scores, the whole beam, overflow, n-best rows and scores, counts,
the stable prefix, committed, the window's frame count, the largest K and the retirable ids), and for every cut the
facts the tests assert before any device call (`cuts`).
"""

import functools

import numpy as np

import golden_util
import primed_ref
import retire_ref
from oracle import oracle
from uisrnn_amd import synth


@functools.lru_cache(maxsize=None)
def model(name):
  oracle.lib()
  return primed_ref.Model(golden_util.load_case(name)['params'])


def speaker_frames(seed, ids, dim, noise=0.05):
  """One frame per entry of ids around that speaker's unit centroid (test_gpu_retire.frames)."""
  rng = np.random.default_rng(seed)
  cent = rng.standard_normal((max(ids) + 1, dim))
  cent /= np.linalg.norm(cent, axis=1, keepdims=True)
  return cent[np.array(ids)] + noise * rng.standard_normal((len(ids), dim))


class Trace:
  """A plan under construction: every operation is applied to the reference as it is appended."""

  def __init__(self, model_name, frames, beam, window=16):
    from test_gpu_retire import want   # pylint: disable=import-outside-toplevel
    self._want = want
    self.model_name, self.frames, self.beam, self.window = model_name, np.asarray(frames, dtype=np.float64), beam, window
    self.ref = retire_ref.Session(model(model_name), beam)
    self.pos = 0
    self.ops, self.results, self.wants, self.cuts = [], [], [], {}

  def _done(self, op, result=None):
    self.ops.append(op)
    self.results.append(result)
    self.wants.append(self._want(self.ref, self.beam))

  def push(self, n):
    assert 1 <= n <= 5 and self.pos + n <= len(self.frames) and self.ref.have + n <= self.window, (n, self.pos, self.ref.have)
    with np.errstate(all='ignore'):
      self.ref.push(self.frames[self.pos:self.pos + n])
    self._done(('push', self.pos, n))
    self.pos += n

  def push_to(self, have):
    """Chunks of 5, 4, 3, ... frames until the window holds `have`."""
    n = 5
    while self.ref.have < have:
      self.push(min(n, have - self.ref.have))
      n = n - 1 if n > 2 else 5

  def commit(self, horizon):
    out = self.ref.commit(None if horizon < 0 else horizon)
    self._done(('commit', horizon), (list(out[0]), out[1]))
    return out

  def retire(self):
    self._done(('retire',), self.ref.retire(self.ref.retirable()))
    return self.results[-1]

  def prime(self, n, source='greedy'):
    assert self.ref.received == 0 and self.pos == 0
    frames = self.frames[:n]
    labels = np.array([int(v) for v in oracle.decode(model(self.model_name).params, [frames], 1, 1, 1)['labels'][0]], dtype=np.int32)
    start = primed_ref.advance_forced(model(self.model_name), frames, labels)
    self.ref = retire_ref.Session(model(self.model_name), self.beam, start)
    self.pos = n
    self._done(('prime', n, labels), int(np.float32(start.score).view(np.uint32)))

  def cut(self, name):
    ref = self.ref
    assert name not in self.cuts, name
    self.cuts[name] = {'at': len(self.ops), 'N': ref.have, 'committed': ref.committed, 'live': len(ref.beam), 'K': ref.K(),
                       'gone': list(ref.gone), 'received': ref.received}
    self._done(('cut', name))


@functools.lru_cache(maxsize=None)
def continuation(beam, window=16, model_name='tiny_d16', seed=4242):
  """The cut states of one stream in a window of `window` frames: nothing received; N = 1, 2, 3 and 5; a full
  window; after a commit with a horizon that pruned (live < beam, committed > 0); a window a commit just emptied;
  and a few pushes and commits behind each."""
  dim = int(model(model_name).params['observation_dim'])
  t = Trace(model_name, synth.make_utterance(seed, 4 * window + 40, dim, mean_segment=4.0)[0], beam, window)
  t.cut('fresh')
  for n, name in ((1, 'N1'), (1, 'N2'), (1, 'N3'), (2, 'N5')):
    t.push(n)
    t.cut(name)
  t.push_to(window)
  t.cut('full')
  t.commit(8)
  t.cut('committed')
  t.push(3 if (t.ref.have + 3) % 2 == 0 else 2)
  t.commit(0)
  t.cut('emptied')
  t.push(4)
  t.push(5)
  t.commit(6)
  t.push(3)
  t.push(1)
  t.commit(-1)
  t.push(2)
  return t


@functools.lru_cache(maxsize=None)
def primed(beam, model_name='tiny_d16', seed=99):
  dim = int(model(model_name).params['observation_dim'])
  t = Trace(model_name, synth.make_utterance(seed, 40, dim, mean_segment=4.0)[0], beam)
  t.prime(6)
  t.cut('primed')
  t.push(3)
  t.push(5)
  t.commit(6)
  t.push(4)
  return t


@functools.lru_cache(maxsize=None)
def retired(beam, model_name='tracker_d64_h300'):
  """test_gpu_retire's 'old' utterance: speaker 0 is left behind by a commit and retired; later a new speaker and
  then speaker 0 again, who must get ids nobody ever had."""
  ids = [0, 0, 0, 1, 1, 2, 2] + [1, 1, 1, 2, 2, 2] * 2 + [3, 3, 3] + [0, 0, 0, 1, 1, 1, 1, 2]
  t = Trace(model_name, speaker_frames(101, ids, 64), beam)
  t.push(4)
  t.push(3)
  t.commit(3)
  t.retire()
  t.cut('retired')
  for n in (1, 3, 5):
    t.push(n)
  t.commit(4)
  for n in (3, 3, 3, 2):
    t.push(n)
  t.commit(4)
  t.push(3)
  return t


@functools.lru_cache(maxsize=None)
def at_the_cap(beam, model_name='tracker_d64_h300'):
  """Five speakers, two frames each, then a cut: the target's max_clusters is the largest K of the beam there; the
  frames that follow bring new speakers."""
  ids = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4] + [5, 5, 6, 6, 7, 7]
  t = Trace(model_name, speaker_frames(202, ids, 64), beam)
  for n in (4, 3, 3):
    t.push(n)
  t.cut('at_cap')
  for n in (2, 2, 2):
    t.push(n)
  return t


@functools.lru_cache(maxsize=None)
def short(beam, model_name, first=5):
  """Other model shapes and session paths: two cuts (an odd window; a committed part) in fourteen frames of the golden
  case's first sequence; pushes of four and five frames take the one-launch kernel where the session has it."""
  t = Trace(model_name, golden_util.load_case(model_name)['seqs'][0][:24], beam)
  t.push(first)
  t.cut('odd')
  t.push(4)
  t.commit(4)
  t.cut('committed')
  t.push(4)
  t.push(1)
  return t


@functools.lru_cache(maxsize=None)
def endless(beam=4, window=16, horizon=8, frames=200, more=40, model_name='tiny_d16', seed=777):
  """A stream of `frames` frames through a window of `window` with commit(horizon) whenever the next chunk does not
  fit, a cut, and `more` frames behind it in the same way."""
  dim = int(model(model_name).params['observation_dim'])
  t = Trace(model_name, synth.make_utterance(seed, frames + more, dim, mean_segment=4.0)[0], beam, window)

  def feed(upto):
    while t.pos < upto:
      n = min(5, upto - t.pos)
      if t.ref.have + n > window:
        t.commit(horizon)
      t.push(n)

  feed(frames)
  t.cut('long')
  feed(frames + more)
  return t
