"""tests/decode_ref64.py held to the reference's recordings, the oracle held to decode_ref64 in every hostile
regime, and the functions of include/uis_numerics.h held to double libm.  No GPU.

The recordings are torch float32: the tolerances on them are float32 round-off on the recorded magnitudes
(rtol 2e-6, atol 1e-6 on CoreRNN rows, 1e-5 relative on NLLs).  The oracle-against-float64 tolerance is the a
priori bound decode_ref64 computes from its own float64 run (see its docstring): nothing here is fitted to
what the oracle returns.
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

import decode_ref64
import forced_ref
import golden_util
import hostile
from uisrnn_amd import synth, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params_of(name):
  if name.endswith('.uisrnn'):
    return weights.load_checkpoint(os.path.join(golden_util.GOLDEN_DIR, name))
  if name.startswith('trained_'):
    return golden_util.load_trained(name)['params']
  return golden_util.load_case(name)['params']


# ---- the reference is right

@pytest.mark.parametrize('name', golden_util.case_names())
def test_reference_unit_rows(name):
  """CoreRNN.forward and weighted_mse_loss as the reference computed them (unit_* / mse_* of every fixture)."""
  case = golden_util.load_case(name)
  unit = case['unit']
  for x, h, mean_ref, h_ref in zip(unit['unit_x'], unit['unit_h'], unit['unit_mean'], unit['unit_hout']):
    mean, hout, _ = decode_ref64.step(case['params'], x, h)
    np.testing.assert_allclose(mean, mean_ref, rtol=2e-6, atol=1e-6)
    np.testing.assert_allclose(hout, h_ref, rtol=2e-6, atol=1e-6)
  for a, b, val in zip(unit['mse_a'], unit['mse_b'], unit['mse_val']):
    got = decode_ref64.weighted_mse(case['params'], a, b)
    if np.isfinite(val):
      assert abs(got - float(val)) <= 1e-5 * abs(float(val)), (got, val)
    else:
      assert np.isnan(got) if np.isnan(val) else got == float(val), (got, val)


def test_reference_forced_scores():
  """The reference's neg_likelihood of given labelings (fn_forced_scores.npz), 1e-5 relative."""
  data = np.load(os.path.join(golden_util.GOLDEN_DIR, 'fn_forced_scores.npz'))
  worst = 0.0
  for case in [str(c) for c in data['cases']]:
    params = _params_of(str(data[case + '/checkpoint']))
    dim = int(params['observation_dim'])
    lens = [int(n) for n in data[case + '/lengths']]
    seqs = [synth.make_utterance(int(data[case + '/utt_seed']) + u, n, dim)[0] for u, n in enumerate(lens)]
    bounds = np.concatenate([[0], np.cumsum(lens)])
    for k in range(int(data[case + '/n_labelings'])):
      labels = data['{}/labels_{}'.format(case, k)]
      ref = data['{}/scores_{}'.format(case, k)]
      for u, seq in enumerate(seqs):
        got, _ = decode_ref64.forced_nll(params, seq, labels[bounds[u]:bounds[u + 1]])
        if np.isfinite(ref[u]):
          rel = abs(got - ref[u]) / abs(ref[u])
          worst = max(worst, rel)
          assert rel <= 1e-5, (case, k, u, got, ref[u])
        else:
          assert got == ref[u], (case, k, u, got, ref[u])
  print('worst relative difference to the recorded neg_likelihoods: {:.3g}'.format(worst))


def test_reference_calculate_score_arrays():
  """_calculate_score's arrays (fn_scores.npz) of the look_ahead 1 decodes, every window: the beam is replayed
  from the RECORDED scores (which candidates survived, uisrnn.py:546-559), each survivor is a forced trace, and
  every finite recorded candidate must be that trace's neg_likelihood plus the candidate's loss.  Of the
  look_ahead 2 decodes the first window (an empty beam state: the labelings (0, 0) and (0, 1))."""
  data = np.load(os.path.join(golden_util.GOLDEN_DIR, 'fn_scores.npz'))
  worst, checked = 0.0, 0
  for i in range(int(data['n_cases'])):
    name = str(data['case_{}'.format(i)][0])
    utt, keep, beam, look, tau, _ = [int(v) for v in data['cfg_{}'.format(i)]]
    case = golden_util.load_trained(name) if name.startswith('trained_') else golden_util.load_case(name)
    params = case['params']
    seq = np.tile(np.asarray(case['seqs'][utt], dtype=np.float64)[:keep], (tau, 1))
    rec = data['scores_{}'.format(i)]
    if look == 2:
      for c0, c1 in ((0, 0), (0, 1)):
        got, _ = decode_ref64.forced_nll(params, seq[:2], [c0, c1])
        assert abs(got - rec[0, 0, c0, c1]) <= 1e-5 * abs(rec[0, 0, c0, c1]), (name, c0, c1)
        checked += 1
      assert np.isposinf(rec[0, 0, 1:, :]).all() and np.isposinf(rec[0, 1:]).all()
      continue
    n_win = min(rec.shape[0], 8 if int(params['rnn_hidden_size']) >= 256 else rec.shape[0])
    states = [decode_ref64.Forced(params)]
    for w in range(n_win):
      nxt = {}
      for r, state in enumerate(states):
        for c in range(len(state.means) + 1):
          new, _, _ = state.advance(seq[w], c)
          want = float(rec[w, r, c])
          assert np.isfinite(want), (name, w, r, c)
          rel = abs(new.total - want) / abs(want)
          worst = max(worst, rel)
          assert rel <= 1e-5, (name, w, r, c, new.total, want)
          nxt[(r, c)] = new
          checked += 1
        assert np.isposinf(rec[w, r, len(state.means) + 1:]).all(), (name, w, r)
      assert np.isposinf(rec[w, len(states):]).all(), (name, w)
      flat = rec[w].ravel()
      order = np.argsort(flat, kind='stable')[:beam]
      states = [nxt[tuple(int(v) for v in np.unravel_index(j, rec[w].shape))] for j in order if np.isfinite(flat[j])]
  assert checked > 500
  print('{} recorded candidate scores, worst relative difference {:.3g}'.format(checked, worst))


# ---- the oracle against float64, per regime

@pytest.mark.parametrize('regime', hostile.REGIMES)
@pytest.mark.parametrize('dim,hidden,depth', hostile.SHAPES, ids=lambda v: str(v))
def test_oracle_within_the_a_priori_bound(dim, hidden, depth, regime, oracle_lib):
  """oracle.rnn_step and forced_ref.score against decode_ref64, within the bound decode_ref64 derives from its
  own run; the regime's `reached` check first."""
  beam = 6
  case = hostile.build(regime, dim, hidden, depth, lengths=(12, 9, 15, 8), offset=3 * hidden)
  ref = oracle_lib.decode(case.params, case.seqs, beam, 1, 1, n_threads=4)
  hostile.reached(case, oracle_lib, ref, beam)
  rows = hostile.step_rows(case, oracle_lib)
  w_step = hostile.check_step(case, rows, lambda x, h: oracle_lib.rnn_step(case.params, x, h))
  w_forced = 0.0
  for labels in hostile.labelings(case, ref).values():
    scores, losses = forced_ref.score(case.params, case.seqs[:2], labels[:2])
    ratio, used, seen = hostile.check_forced(case, labels, scores, losses, utterances=(0, 1))
    w_forced = max(w_forced, ratio)
    frames = '{} of {} frames'.format(used, seen)
    # (the one case with nothing to compare: two layers at gain 200, where even the first frame's bound, that of the
    # new-cluster constant, is 0.9 of the loss)
    assert used > 0 or (regime == 'saturated200' and depth == 2), (used, seen)
  print('{} D {} H {} depth {}: error / bound  rnn_step {:.3g}  forced NLL {:.3g} ({} under a bound that bites)'.format(
      regime, dim, hidden, depth, w_step, w_forced, frames))


def test_edges_cover_the_whole_list_on_the_small_models():
  """Hidden sizes below len(EDGES) see a slice of the list per gate.  Over the offsets the GPU tests use on the
  k_decode_small shapes, what the float64 run hands to the r gate's sigmoid, to the z gate's sigmoid and to the n
  gate's tanh covers every edge, as float32 bits."""
  want = set(hostile.EDGES_SEEN.view(np.uint32).tolist())
  seen = [set(), set(), set()]
  for dim, hidden, depth, offset in hostile.SMALL_EDGE_CASES:
    case = hostile.build('edges', dim, hidden, depth, lengths=(9, 8), offset=offset)
    for acc, got in zip(seen, hostile.gate_arguments(case)):
      acc |= got
  for gate, acc in zip('rzn', seen):
    assert want <= acc, (gate, len(want - acc))


# ---- the header's functions

_SWEEP_C = r'''
#include <stdio.h>
#include <string.h>
#include <math.h>
#include "uis_numerics.h"

static double ulp_of(double ref) {           /* one float32 ulp at |ref| */
  double a = fabs(ref);
  if (a < 1.17549435082228750797e-38) return 1.40129846432481707092e-45;
  int e;
  frexp(a, &e);
  return ldexp(1.0, e - 24);
}

static double worst[3];
static float worst_at[3];

static void probe(float x) {
  double refs[3] = { exp((double)x), 1.0 / (1.0 + exp(-(double)x)), tanh((double)x) };
  float got[3] = { uis_expf(x), uis_sigmoidf(x), uis_tanhf(x) };
  for (int f = 0; f < 3; ++f) {
    double err = fabs((double)got[f] - refs[f]) / ulp_of(refs[f]);
    if (!(err <= worst[f])) { worst[f] = err; worst_at[f] = x; }
  }
}

int main(int argc, char** argv) {
  /* every 61st bit pattern of either sign with |x| <= 87, then the edge list given on the command line */
  unsigned long n = 0;
  for (uint32_t u = 0; u <= 0x42ae0000u; u += 61) {
    probe(uis_bits2f(u));
    probe(uis_bits2f(u | 0x80000000u));
    n += 2;
  }
  for (int i = 1; i < argc; ++i) {
    uint32_t u;
    sscanf(argv[i], "%x", &u);
    float x = uis_bits2f(u);
    if (fabsf(x) <= 87.0f) { probe(x); ++n; }
    printf("edge %08x %08x %08x %08x\n", u, uis_f2bits(uis_expf(x)), uis_f2bits(uis_sigmoidf(x)), uis_f2bits(uis_tanhf(x)));
  }
  printf("swept %lu\n", n);
  printf("worst exp %.4f %a sigmoid %.4f %a tanh %.4f %a\n", worst[0], worst_at[0], worst[1], worst_at[1], worst[2], worst_at[2]);
  return 0;
}
'''


def _f32_bits(v):
  return int(np.array([v], dtype=np.float32).view(np.uint32)[0])


def test_header_functions_against_double_libm(tmp_path):
  """uis_expf / uis_sigmoidf / uis_tanhf of include/uis_numerics.h, compiled as the oracle compiles them:
  at most 1 / 3 / 4 ulp from double libm on |x| <= 87 (every 61st bit pattern and hostile.EDGES), and the exact
  values at the clamps.  The device test (tests/test_gpu_hostile.py) leans on this contract."""
  gcc = shutil.which('gcc') or shutil.which('cc')
  assert gcc, 'a C compiler is needed (the oracle is built with one)'
  src = tmp_path / 'sweep.c'
  src.write_text(_SWEEP_C)
  exe = tmp_path / 'sweep'
  subprocess.check_call([gcc, '-O2', '-std=gnu11', '-mavx2', '-mfma', '-ffp-contract=off', '-fno-math-errno',
                         '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe), '-lm'])
  extra = np.array([88.0, -88.0, 89.0, -89.0, 1e30, -1e30, np.inf, -np.inf], dtype=np.float32)
  edges = np.concatenate([hostile.EDGES, extra])
  out = subprocess.run([str(exe)] + ['{:08x}'.format(_f32_bits(v)) for v in edges], stdout=subprocess.PIPE, text=True,
                       check=True, timeout=300).stdout
  lines = out.strip().splitlines()
  words = lines[-1].split()
  ulps = {words[1]: float(words[2]), words[4]: float(words[5]), words[7]: float(words[8])}
  print(lines[-2], '\n', lines[-1])
  assert int(lines[-2].split()[1]) > 36_000_000     # (every 61st pattern up to 87.0, both signs)
  assert ulps['exp'] <= 1.0 and ulps['sigmoid'] <= 3.0 and ulps['tanh'] <= 4.0, lines[-1]
  table = {}
  for line in lines:
    if line.startswith('edge'):
      _, x, e, s, t = line.split()
      table[int(x, 16)] = (int(e, 16), int(s, 16), int(t, 16))
  e88 = _f32_bits(np.exp(np.float64(88.0)))           # exp clamps to [-87, 88]: normal results, never inf or 0
  e87 = _f32_bits(np.exp(np.float64(-87.0)))
  for x in (88.5, 89.0, 100.0, 1e30, np.inf):
    assert abs(table[_f32_bits(x)][0] - e88) <= 1, x
    assert table[_f32_bits(x)][0] == table[_f32_bits(88.0)][0], x
    assert abs(table[_f32_bits(-x)][0] - e87) <= 1, x
    assert table[_f32_bits(-x)][0] == table[_f32_bits(-87.0)][0], x
    # a saturated gate: sigmoid(-88 and below) is ONE subnormal, sigmoid(88 and above) exactly 1
    assert table[_f32_bits(-x)][1] == _f32_bits(6.0546015e-39), x
    assert table[_f32_bits(x)][1] == _f32_bits(1.0), x
    assert table[_f32_bits(x)][2] == _f32_bits(1.0) and table[_f32_bits(-x)][2] == _f32_bits(-1.0), x
  assert table[_f32_bits(-88.0)][1] == _f32_bits(6.0546015e-39)
  assert 0 < np.array([table[_f32_bits(-88.0)][1]], dtype=np.uint32).view(np.float32)[0] < 2.0 ** -126
  assert table[_f32_bits(0.0)][2] == _f32_bits(0.0) and table[_f32_bits(-0.0)][2] == _f32_bits(-0.0)   # sign kept
  for x in (1e-40, -1e-40, 1.4e-45, -1.4e-45):       # tanh of a subnormal is that subnormal
    assert table[_f32_bits(x)][2] == _f32_bits(x), x
  assert table[_f32_bits(0.0)][1] == _f32_bits(0.5) and table[_f32_bits(-0.0)][1] == _f32_bits(0.5)
