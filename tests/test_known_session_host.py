"""Known speakers in streaming sessions, the CPU side: the reference of tests/known_session_ref.py against the references
it is built from, the facts the GPU cases of tests/test_gpu_known_session.py rely on, the Python front end's keyword
checks and name tables against a stand-in decoder, and csrc/uis_blob.h's validator on tagged blobs (stand-alone, also
under the host compiler's sanitizers).  No GPU needed.
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

import commit_ref
import known_ref
import known_session_cases as kc
import known_session_ref as ksr
import retire_ref
import test_restart_host as rh
import uisrnn_amd
from uisrnn_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _final(name, plan):
  return kc.trace(name, plan)[-1]['snap']


# ---- 1. the reference against the references it is built from

@pytest.mark.parametrize('name', ['small4', 'deep'])
def test_without_tags_and_with_all_zero_tags_it_is_the_untagged_session(name, oracle_lib):
  sh = kc.shape(name)
  plain, zeros = _final(name, 'plain'), _final(name, 'zeros')
  assert plain == zeros
  for u, n in enumerate(kc.chunk_lengths(sh)):
    seq = sh.pool[u][0][0][:n]
    for cls in (commit_ref.Session, retire_ref.Session):
      ref = cls(sh.model, sh.beam)
      for t0 in range(0, n, 3):
        ref.push(seq[t0:t0 + 3])
      assert ref.rows().tolist() == plain[u]['rows'] and _bits(ref.scores()).tolist() == plain[u]['scores'], (name, u)
    assert plain[u]['bind'] == [0] + [-1] * 127 and plain[u]['tagged'] == []


def test_a_commit_and_a_retirement_without_tags_are_retire_refs(oracle_lib):
  sh = kc.shape('small4')
  seq = sh.pool[0][0][0]
  a, b = ksr.Session(sh.model, sh.beam), retire_ref.Session(sh.model, sh.beam)
  for s in (a, b):
    s.push(seq[:12])
    s.commit(2)
    s.push(seq[12:15])
    s.commit(0)
  assert a.retirable() == b.retirable() and a.retirable(), 'nothing retirable: the comparison is vacuous'
  assert a.retire(a.retirable()[:1]) == b.retire(b.retirable()[:1])
  for s in (a, b):
    s.push(seq[15:20])
  assert a.rows().tolist() == b.rows().tolist() and _bits(a.scores()).tolist() == _bits(b.scores()).tolist()
  assert a.labels() == b.labels()


@pytest.mark.parametrize('name', kc.SHAPES)
def test_pushed_whole_it_is_the_offline_decode_and_the_tags_matter(name, oracle_lib):
  sh = kc.shape(name)
  snap = _final(name, 'chunk_whole')
  changed = 0
  for u, n in enumerate(kc.chunk_lengths(sh)):
    want = known_ref.decode(sh.model, sh.pool[u][0][0][:n], sh.beam, tags=kc.life_tags(u, 0, kc.SEQ_LEN)[:n])
    assert snap[u]['rows'][0] == want['labels'].tolist(), (name, u)
    assert snap[u]['scores'][0] == int(_bits(want['score'])[0])
    assert _bits(np.array([h.score for h in want['beam']])).tolist() == snap[u]['scores']
    assert snap[u]['bind'][1:4] == [known_ref.tags_of(want['beam'][0]).index(g) if g in known_ref.tags_of(want['beam'][0]) else -1
                                    for g in (1, 2, 3)]
    # the facts the GPU cases rely on
    assert snap[u]['live'] > 0, 'an empty beam'
    assert snap[u]['K'] < sh.cap and want['max_clusters'] < sh.cap, 'the cluster cap is in reach'
    changed += snap[u]['rows'][0] != kc.untagged_rows(name)[u]
  assert 4 * changed >= sh.n_utt, 'the tags change {} of {} slots: the comparison would be vacuous'.format(changed, sh.n_utt)


@pytest.mark.parametrize('plan', ['commit', 'restart', 'tag127', 'all_bound', 'together'])
@pytest.mark.parametrize('name', kc.SHAPES)
def test_no_plan_empties_a_beam_or_reaches_the_cap(name, plan, oracle_lib):
  sh = kc.shape(name)
  for st in kc.trace(name, plan):
    for u, col in enumerate(st['snap']):
      assert col['K'] < sh.cap and (col['live'] > 0 or col['have'] + col['committed'] == 0), (plan, st['op'], u)
  last = kc.trace(name, plan)[-1]['snap']
  if plan == 'tag127':
    assert all(col['bind'][127] == 0 for col in last)    # the first frame's cluster
  if plan == 'all_bound':
    st = kc.trace(name, plan)
    assert all(col['K'] == 4 and col['bind'][0] == 4 for col in st[3]['snap'])       # every cluster of rank 0 is bound
    assert all(col['bind'][5] == 4 and col['rows'][0][4] == 4 for col in st[4]['snap'])   # the fifth tag opened the new cluster
    assert all(col['rows'][0][5] == col['bind'][2] == 1 for col in st[5]['snap'])     # tag 2 again: its cluster
  if plan == 'together':
    assert all(col['K'] <= lim for col, lim in zip(last, kc.together_limits(sh)))
  if plan == 'restart':
    st = kc.trace(name, plan)
    assert st[0]['snap'][1]['bind'][0] > 0 and st[1]['snap'][1]['bind'][0] == 0 and st[2]['snap'][1]['bind'][1] == 0


@pytest.mark.parametrize('name', kc.SHAPES)
def test_primed_with_tags_it_continues_as_the_offline_decode_from_that_hypothesis(name, oracle_lib):
  sh = kc.shape(name)
  tr = kc.trace(name, 'prime')
  for u in (0, 2):
    lab, n = tr[0]['call']['labels'][u], len(tr[0]['call']['labels'][u])
    at = sum(len(x) for x in tr[0]['call']['labels'][:u] if x is not None)
    g = tr[0]['call']['speakers'][at:at + n]
    assert g.any() and len(set(lab.tolist())) > 1, 'the prefix binds nothing'
    seq = sh.pool[u][0][0]
    start = ksr.primed(sh.model, seq[:n], lab, g)
    want = known_ref.decode(sh.model, seq[n:n + 6], sh.beam, tags=kc.life_tags(u, 0, kc.SEQ_LEN)[n:n + 6], start=start)
    col = tr[-1]['snap'][u]
    assert col['rows'] == [h.trace for h in want['beam']] and col['scores'] == _bits([h.score for h in want['beam']]).tolist()
    assert tr[0]['result'][u] == int(_bits(start.score)[0])
    assert tr[0]['snap'][u]['bind'][0] == len(set(g.tolist()) - {0})


def test_the_prime_contradiction_rule():
  assert ksr.bind_prefix([0, 0, 1, 1, 2], [0, 3, 0, 1, 0]) == (3, 1, 0)
  assert ksr.bind_prefix([0, 1, 0], [7, 0, 7]) == (7, 0)
  assert ksr.bind_prefix([0, 1], [0, 0]) == (0, 0)
  for labels, tags in (([0, 1], [3, 3]), ([0, 0], [3, 4]), ([0, 1, 0], [2, 5, 5])):
    with pytest.raises(ValueError, match='contradict'):
      ksr.bind_prefix(labels, tags)


@pytest.mark.parametrize('name', kc.SHAPES)
def test_the_retire_case_holds_what_it_is_for(name, oracle_lib):
  tr = kc.trace(name, 'retire')
  sh = kc.shape(name)
  before, after = tr[3], tr[5]
  assert before['kind'] == 'query' and after['kind'] == 'query'
  # a retirable untagged cluster below a tagged one, and a tagged cluster that would be retirable but for its tag
  plain = retire_ref.Session.retirable(_slot0_session(sh, tr))
  assert before['result']['retirable'][0] == [0] and before['result']['tagged'][0] == [1] and plain == [0, 1]
  assert before['snap'][0]['bind'][5] == 1 and after['snap'][0]['bind'][5] == 0     # the binding follows its cluster
  assert after['result']['retirable'][0] == [] and after['result']['tagged'][0] == [0]
  for st in tr[6:8]:                                                               # the next tagged frames land on it
    assert st['kind'] == 'tag' and st['snap'][0]['rows'][0][-1] == 0
  assert all(col['live'] > 0 and col['K'] < sh.cap for st in tr for col in st['snap'] if col['have'] + col['committed'])


def _slot0_session(sh, tr):
  """Slot 0 of the retire plan as the trace's first query finds it, rebuilt: primed, its window emptied by the commit."""
  call = tr[0]['call']
  s = ksr.Session(sh.model, sh.beam, ksr.primed(sh.model, call['chunks'][0], call['labels'][0], call['speakers']))
  s.commit(0)
  return s


# ---- 2. the front end, against a stand-in decoder

class _Tagged(rh._StandIn):   # pylint: disable=protected-access
  """test_restart_host's stand-in that records the speakers tables it is handed; every tag g is bound to cluster g - 1."""

  def __init__(self, n_utt):
    super().__init__(n_utt)
    self.tables, self.seen = [], [set() for _ in range(n_utt)]

  def _take(self, chunks, speakers):
    sizes = [0 if c is None else len(c) for c in chunks]
    self.tables.append(None if speakers is None else np.array(speakers))
    if speakers is not None:
      assert speakers.dtype == np.uint8 and speakers.shape == (sum(sizes),)
      at = 0
      for u, n in enumerate(sizes):
        self.seen[u] |= set(speakers[at:at + n].tolist()) - {0}
        at += n

  def stream_push(self, chunks, speakers=None):   # pylint: disable=arguments-differ
    self._take(chunks, speakers)
    super().stream_push(chunks)

  def stream_prime(self, chunks, labels, speakers=None):   # pylint: disable=arguments-differ
    self._take(chunks, speakers)
    return super().stream_prime(chunks, labels)

  def stream_bindings(self):
    out = np.full((len(self.have), 128), -1, dtype=np.int32)
    for u, tags in enumerate(self.seen):
      out[u, 0] = len(tags)
      for g in tags:
        out[u, g] = g - 1
    return out

  def stream_restart(self, which):
    for u, w in enumerate(which):
      if w:
        self.seen[u] = set()
    return super().stream_restart(which)

  def stream_export(self, u):
    with open(self.blob_path, 'rb') as f:
      return f.read()

  def stream_import(self, u, blob):
    self.imported = (u, bytes(blob))


def _session(n_utt):
  session = rh._session(n_utt, 100)   # pylint: disable=protected-access
  session._decoder = _Tagged(n_utt)   # pylint: disable=protected-access
  return session


def test_push_numbers_names_by_first_appearance_across_pushes():
  s = _session(3)
  dec = s._decoder   # pylint: disable=protected-access
  s.push([np.zeros((3, 4)), np.zeros((2, 4)), None], known_speakers=[['ann', None, 'bob'], None, None])
  assert dec.tables[-1].tolist() == [1, 0, 2, 0, 0]
  s.push([np.zeros((2, 4)), None, np.zeros((2, 4))], known_speakers=[['bob', ('c', 1)], None, [7, 7]])
  assert dec.tables[-1].tolist() == [2, 3, 1, 1]
  assert s.speaker_names(0) == ['ann', 'bob', ('c', 1)] and s.speaker_names(1) == [] and s.speaker_names(2) == [7]
  s.push([np.zeros((1, 4)), None, None])                      # no keyword: no table
  assert dec.tables[-1] is None
  s.push([np.zeros((1, 4)), None, None], known_speakers=[None, None, None])   # nobody known: an all-zero table
  assert dec.tables[-1].tolist() == [0]
  assert s.speakers() == [{'ann': 0, 'bob': 1, ('c', 1): 2}, {}, {7: 0}]
  # restart clears that slot's table, and that slot's alone
  s.restart([0])
  assert s.speaker_names(0) == [] and s.speaker_names(2) == [7]
  s.push([np.zeros((1, 4)), None, None], known_speakers=[['bob'], None, None])
  assert dec.tables[-1].tolist() == [1] and s.speakers()[0] == {'bob': 0}
  # prime takes the same keyword and the same table
  s.restart([1])
  s.prime([None, np.zeros((3, 4)), None], [None, ['x', 'x', 'y'], None], known_speakers=[None, ['p', None, 'q'], None])
  assert dec.tables[-1].tolist() == [1, 0, 2] and s.speaker_names(1) == ['p', 'q']


def test_the_keyword_checks_come_before_any_device_work_and_change_nothing():
  s = _session(2)
  dec = s._decoder   # pylint: disable=protected-access
  chunks = [np.zeros((2, 4)), np.zeros((1, 4))]
  s.push(chunks, known_speakers=[['a', 'b'], None])
  for bad, kind, match in (([['a'], None], ValueError, 'has 1 entries for 2 frames'),
                           ([['a', 'b']], ValueError, '1 entries for 2 utterances'),
                           (True, ValueError, 'not a bool'),
                           ([['a', float('nan')], None], ValueError, 'NaN'),
                           ([['a', ['x']], None], TypeError, 'unhashable'),
                           ('ab', ValueError, 'must be a sequence')):
    with pytest.raises(kind, match=match):
      s.push(chunks, known_speakers=bad)
  assert len(dec.tables) == 1 and dec.have.tolist() == [2, 1] and s.speaker_names(0) == ['a', 'b']
  # the 128th name of one utterance, across pushes
  many = _session(1)
  many.push([np.zeros((100, 4))], known_speakers=[list(range(100))])
  many.push([np.zeros((27, 4))], known_speakers=[list(range(100, 127))])
  with pytest.raises(ValueError, match='more than 127 speakers'):
    many.push([np.zeros((2, 4))], known_speakers=[[5, 'one too many']])
  assert len(many._decoder.tables) == 2 and len(many.speaker_names(0)) == 127   # pylint: disable=protected-access
  many.push([np.zeros((1, 4))], known_speakers=[[126]])        # a known name still goes through
  assert many._decoder.tables[-1].tolist() == [127]            # pylint: disable=protected-access


def test_the_pool_takes_names_by_key():
  session = _session(3)
  pool = uisrnn_amd.uisrnn.StreamPool(session)
  pool.open('a')
  pool.open('b')
  pool.push({'a': np.zeros((2, 4)), 'b': np.zeros((1, 4))}, known_speakers={'b': ['zed']})
  assert session._decoder.tables[-1].tolist() == [0, 0, 1]   # pylint: disable=protected-access
  assert pool.speakers('b') == {'zed': 0} and pool.speaker_names('b') == ['zed'] and pool.speakers('a') == {}
  with pytest.raises(ValueError, match='dict'):
    pool.push({'a': np.zeros((1, 4))}, known_speakers=[['x']])


# ---- 3. the blob validator on tagged blobs, and the helper that reads a blob's bytes

def _build_blob_tags(tmp_path, flags):
  cxx = shutil.which(os.environ.get('CXX', '') or 'g++') or shutil.which('c++') or shutil.which('clang++')
  if not cxx:
    pytest.skip('no host C++ compiler')
  exe = str(tmp_path / 'blob_tags')
  subprocess.run([cxx] + flags + ['-I', os.path.join(ROOT, 'uisrnn_amd', 'csrc'), os.path.join(ROOT, 'tests', 'blob_tags_main.cpp'),
                                  '-o', exe], check=True)
  return exe


def test_the_blob_validator_on_tagged_blobs_and_the_python_helper(tmp_path):
  exe = _build_blob_tags(tmp_path, ['-std=c++17', '-O1', '-Wall', '-Wextra'])
  path = str(tmp_path / 'tagged.blob')
  done = subprocess.run([exe, path], capture_output=True, text=True)
  assert done.returncode == 0 and done.stdout.startswith('blob_tags: ok'), (done.returncode, done.stdout, done.stderr)
  with open(path, 'rb') as f:
    blob = f.read()
  assert _capi.blob_max_tag(blob) == 127 and _capi.blob_info(blob)['K'] == 3
  assert sorted(_capi.blob_info(blob)) == ['B', 'K', 'N', 'bytes', 'committed', 'live', 'slots']   # (its dict stays as it is)
  # import_state: more tags in the blob than names given is a ValueError before the library call
  s = _session(2)
  dec = s._decoder   # pylint: disable=protected-access
  dec.blob_path, dec.imported = path, None
  s._final[0] = list(range(40))   # pylint: disable=protected-access  (the blob's committed frames: the trailer must match)
  state = s.export_state(0)
  with pytest.raises(ValueError, match='binds speaker tag 127'):
    s.import_state(1, state)
  with pytest.raises(ValueError, match='binds speaker tag 127'):
    s.import_state(1, state, speaker_names=['a', 'b'])
  assert dec.imported is None
  names = ['n%d' % g for g in range(127)]
  s.import_state(1, state, speaker_names=names)
  assert dec.imported == (1, blob) and s.speaker_names(1) == names
  pool = uisrnn_amd.uisrnn.StreamPool(_session(1))
  pool._session._decoder.imported = None   # pylint: disable=protected-access
  with pytest.raises(ValueError, match='binds speaker tag 127'):
    pool.adopt('k', state)
  assert pool.adopt('k', state, speaker_names=names) == 0 and pool.speaker_names('k') == names


def test_the_blob_validator_on_tagged_blobs_under_the_sanitizers(tmp_path):
  cxx = shutil.which(os.environ.get('CXX', '') or 'g++') or shutil.which('c++') or shutil.which('clang++')
  if not cxx:
    pytest.skip('no host C++ compiler')
  base = ['-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
  probe = str(tmp_path / 'probe.cpp')
  with open(probe, 'w') as f:
    f.write('int main() { return 0; }\n')
  # (as tests/test_migrate_host.py builds blob_check_main.cpp: the runtime inside the program where the compiler offers that)
  for flags in (base + ['-static-libasan', '-static-libubsan'], base + ['-static-libsan'], base):
    if subprocess.run([cxx] + flags + [probe, '-o', str(tmp_path / 'probe')], capture_output=True).returncode == 0:
      break
  else:
    pytest.skip('the host compiler cannot link the sanitizer runtime')
  if subprocess.run([str(tmp_path / 'probe')], capture_output=True).returncode != 0:
    pytest.skip('a program with the sanitizer runtime does not start in this environment')
  exe = _build_blob_tags(tmp_path, flags)
  done = subprocess.run([exe], capture_output=True, text=True)
  assert done.returncode == 0 and done.stdout.startswith('blob_tags: ok'), (done.returncode, done.stdout, done.stderr)


def test_the_symbols_are_declared():
  assert {'uis_stream_speakers', 'uis_stream_bindings'} <= set(_capi.EXPORTED_SYMBOLS)
  assert _capi.UIS_ABI_VERSION == 6
