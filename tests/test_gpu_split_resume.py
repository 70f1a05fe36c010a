"""A decode in two launches whose first launch ends some clusters' utterances altogether.

A launch that stops early leaves every cluster's beam tables in the resume buffer and the next launch reads every
cluster's back (k_decode_rs, k_decode_big<WS>).  A cluster whose utterances have all ended inside the first launch has
no step left, but its tables are read back all the same, and its statistics are flushed by the last launch: they have
to be the tables it ended with, not whatever the buffer held.  A ragged float64 list with short utterances next to
long ones, cut at frame 40: the labels, the final beam and the statistics (rnn rows, candidates, the largest cluster
count) of the two launches are the single launch's, the cluster count the oracle's -- also with the workspace poisoned.
"""

import numpy as np
import pytest

import instantiation_cases as ic
from uisrnn_amd import _capi

pytestmark = pytest.mark.gpu

# utterance u lives on cluster u % 8 of a whole device: clusters 1, 3, 4, 5, 6, 7 hold only utterances that end before the cut
LENGTHS = (130, 5, 140, 3, 9, 2, 7, 4, 135, 6, 8)


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('word', [None, '7f7f7f7f'])
@pytest.mark.parametrize('beam', [10, 7], ids=['shape_class', 'run_time_shape'])
def test_clusters_that_end_inside_the_first_launch(beam, word, oracle_lib, monkeypatch):
  import torch  # (only for the device's compute-unit count)
  if torch.cuda.get_device_properties(0).multi_processor_count % 32:
    pytest.skip('no cluster of 32 compute units: the one-launch kernels do not apply')
  params = ic._params(256, 512, 1, None, 0, 0.02)   # pylint: disable=protected-access
  seqs = [np.asarray(s, dtype=np.float64) for s in ic._utterances(256, LENGTHS, 60, False)]   # pylint: disable=protected-access
  ref = oracle_lib.decode(params, seqs, beam, 1, 1, n_threads=8)
  monkeypatch.setenv('UIS_SPLIT_MIN_MB', '0')
  if word is None:
    monkeypatch.delenv('UIS_POISON_WORKSPACE', raising=False)
  else:
    monkeypatch.setenv('UIS_POISON_WORKSPACE', word)
  dec = _capi.Decoder(params)
  try:
    monkeypatch.setenv('UIS_NO_SPLIT', '1')
    one = dec.decode_f64(seqs, beam, 1, 1, want_beam_scores=True)
    monkeypatch.delenv('UIS_NO_SPLIT')
    monkeypatch.setenv('UIS_SPLIT_FRAMES', '40')
    two = dec.decode_f64(seqs, beam, 1, 1, want_beam_scores=True)
  finally:
    dec.close()
  assert one['stats']['decode_launches'] == 1 and two['stats']['decode_launches'] == 2
  assert one['stats']['decode_kernel'] == two['stats']['decode_kernel'] == 'k_decode_rs'
  assert np.array_equal(two['labels'], np.concatenate(ref['labels']))
  assert np.array_equal(_bits(two['beam_scores']), _bits(ref['beam_scores']))
  assert np.array_equal(_bits(one['beam_scores']), _bits(ref['beam_scores']))
  for key in ('rnn_rows', 'rnn_rows_nodedup', 'candidates', 'max_clusters_seen'):
    assert two['stats'][key] == one['stats'][key], key
  assert two['stats']['max_clusters_seen'] == int(ref['max_clusters'].max())
