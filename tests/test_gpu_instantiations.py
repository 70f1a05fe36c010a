"""Every instantiation of the one-launch decode kernels, named by the library, against the oracle bit for bit.

uis_decoder.hip's kernel tables hold some sixty separately compiled kernels.  For every entry (a row of
tests/instantiation_cases.py, which tests/test_instantiation_cases_host.py ties to the library's own enumeration) and
each of its models -- the exact one, and the barely padded ones with the most dead lanes and rows -- one decode:
  * the library reports exactly that entry (Decoder.last_instantiation: family, Hp, Dp, variant, the persist bit),
    unconditionally: a decode that falls back, or a planner that stops picking a shape class, fails here;
  * labels, scores and the whole final beam are the oracle's bits, max_clusters_seen the oracle's;
  * the launch-per-step path (UIS_FLAG_STEPWISE) gives the same bits and evaluates the same number of rnn rows;
  * on the shape-class rows (and once in the families without one) UIS_FLAG_NO_DEDUP gives the same bits.
The persist rows are UIS_FLAG_PERSISTENT sessions fed in uneven pushes, against the oracle's offline decode and a
UIS_FLAG_STEPWISE session; they need a whole MI355X.  The utterance counts follow the device's XCD count.
"""

import numpy as np
import pytest

import instantiation_cases as ic
from uisrnn_amd import _capi

pytestmark = pytest.mark.gpu


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _n_cu():
  import torch  # (only for the device's compute-unit count)
  return torch.cuda.get_device_properties(0).multi_processor_count


def _ncl():
  """Clusters of 32 compute units, as cluster_geometry (uis_decoder.hip) counts them."""
  n_cu = _n_cu()
  return n_cu // 32 if n_cu >= 32 and n_cu % 32 == 0 and n_cu // 32 <= 16 else 0


def _same_as_oracle(case, out_labels, scores, beam_scores, ref, what):
  for u, want in enumerate(ref['labels']):
    assert np.array_equal(out_labels[u], want), '%s: labels differ, utterance %d' % (what, u)
  assert np.array_equal(_bits(scores), _bits(ref['scores'])), what + ': scores'
  assert np.array_equal(_bits(beam_scores), _bits(ref['beam_scores'])), what + ': final beam'


def _decode_case(case, ncl, oracle_lib):
  seqs = case.utterances(ncl)
  ref = oracle_lib.decode(case.params(), seqs, case.beam, case.look_ahead, case.test_iteration, n_threads=8)
  frames, offsets = oracle_lib.pack(seqs)
  dec = _capi.Decoder(case.params())
  try:
    outs = {}
    variants = [case.flags, case.flags | _capi.UIS_FLAG_STEPWISE]
    if case.nodedup:
      variants.append(case.flags | _capi.UIS_FLAG_NO_DEDUP)
    for flags in variants:
      out = dec.decode(frames, offsets, case.beam, case.look_ahead, case.test_iteration, max_clusters=case.cap,
                       flags=flags, want_beam_scores=True)
      what = '%s flags %#x' % (case.name, flags)
      assert out['status'] == 0 and not out['overflow'].any(), what
      inst = dec.last_instantiation()
      if flags & _capi.UIS_FLAG_STEPWISE:
        assert inst == ('stepwise',) + case.row[1:3] + (0, 0), (what, inst)
      else:
        assert inst == case.row, (what, inst)
        assert _capi.DECODE_KERNELS[out['stats']['decode_kernel_code'] & 0xff] == case.row[0], what
      labels = [out['labels'][offsets[u]:offsets[u + 1]] for u in range(len(seqs))]
      _same_as_oracle(case, labels, out['scores'], out['beam_scores'], ref, what)
      assert out['stats']['max_clusters_seen'] == int(ref['max_clusters'].max()), what
      outs[flags] = out
    one, step = outs[variants[0]], outs[variants[1]]
    assert one['stats']['rnn_rows'] == step['stats']['rnn_rows'], case.name
  finally:
    dec.close()


def _run_session(dec, case, seqs, pushes, flags):
  """The session's final labels, scores, beams, and the instantiation reported after every push."""
  dec.stream_begin(len(seqs), case.beam, max(len(s) for s in seqs), max_clusters=case.cap, flags=flags)
  try:
    pos = [0] * len(seqs)
    picks = []
    for take in pushes:
      chunks = [np.asarray(s[p:p + n], dtype=np.float32) if n else None for s, p, n in zip(seqs, pos, take)]
      pos = [p + n for p, n in zip(pos, take)]
      dec.stream_push(chunks)
      picks.append(dec.last_instantiation())
    labels, scores, overflow, status = dec.stream_labels()
    beam = np.empty((len(seqs), case.beam), dtype=np.float32)
    dec._check(dec._lib.uis_last_decode_info(dec._handle, None, beam.ctypes.data_as(_capi._fp)), 'info')  # pylint: disable=protected-access
  finally:
    dec.stream_end()
  assert status == 0 and not overflow.any(), case.name
  return labels, scores, beam, picks


def _session_case(case, ncl, oracle_lib):
  seqs = case.utterances(ncl)
  pushes = case.pushes(ncl)
  ref = oracle_lib.decode(case.params(), seqs, case.beam, 1, 1, n_threads=8)
  hp, dp = case.row[1:3]
  dec = _capi.Decoder(case.params())
  try:
    labels, scores, beam, picks = _run_session(dec, case, seqs, pushes, _capi.UIS_FLAG_PERSISTENT)
    assert set(picks) == {case.row}, (case.name, picks)
    _same_as_oracle(case, labels, scores, beam, ref, case.name + ' persistent')
    # the launch-per-step session, and the plain one (a launch of k_decode_resident per push of four steps or more)
    labels, scores, beam, picks = _run_session(dec, case, seqs, pushes, _capi.UIS_FLAG_STEPWISE)
    assert set(picks) == {('stepwise', hp, dp, 0, 0)}, (case.name, picks)
    _same_as_oracle(case, labels, scores, beam, ref, case.name + ' stepwise')
    labels, scores, beam, picks = _run_session(dec, case, seqs, pushes, 0)
    assert picks[0] == ('k_decode_resident', hp, dp, 0, 0), (case.name, picks)
    assert set(picks) <= {('k_decode_resident', hp, dp, 0, 0), ('stepwise', hp, dp, 0, 0)}, (case.name, picks)
    _same_as_oracle(case, labels, scores, beam, ref, case.name + ' plain')
  finally:
    dec.close()


@pytest.mark.parametrize('row', ic.ROWS, ids=[ic.row_id(row) for row in ic.ROWS])
def test_instantiation_against_the_oracle(row, oracle_lib):
  ncl = _ncl()
  if ncl == 0:
    pytest.skip('no cluster of 32 compute units: the one-launch kernels do not apply')
  if row[4] and _n_cu() != 256:
    pytest.skip('not a whole MI355X')
  for case in ic.CASES[row]:
    if case.session:
      _session_case(case, ncl, oracle_lib)
    else:
      _decode_case(case, ncl, oracle_lib)
