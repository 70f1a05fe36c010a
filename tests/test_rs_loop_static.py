"""k_decode_rs's scalar register diet, checked without a GPU: the spill count of the fixed-shape class and what its step
loop is made of, from one cross-compile of the decoder's device code (tools/loop_census.py, tools/resource_table.py).

What the gain rests on is fragile by nature -- every field of RsArgs is moved into scalar registers of its own by hand
(rs_own_args, uis_select_rs.hip), and a field left out, or a compiler that sees through the move, brings back the
16-register tuples that are spilled and reloaded whole.  The bounds: before that change the kernel had 121 spilled SGPRs
and 237 v_readlane / v_writelane in its loop, with it 67 and 102; a bound half way between them tells the two states
apart and leaves a compiler update room."""

import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

FIXED = '_Z11k_decode_rsILi512ELi256ELi10ELi16EE'


@pytest.fixture(scope='module')
def device_build(tmp_path_factory):
  import loop_census
  from uisrnn_amd import build as hip_build
  tmp = tmp_path_factory.mktemp('census')
  asm = str(tmp / 'decoder.s')
  flags = [f for f in hip_build.FLAGS if f not in ('-shared', '-fPIC')]
  cmd = [hip_build.hipcc()] + flags + ['--cuda-device-only', '-S', '-Rpass-analysis=kernel-resource-usage',
                                       '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'uisrnn_amd', 'csrc'),
                                       hip_build.SOURCES[0], '-o', asm]
  log = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode()
  return loop_census, open(asm).read(), log


def _resources(log, prefix):
  rows, cur = {}, None
  for line in log.splitlines():
    m = re.search(r'Function Name: (\S+)', line)
    if m:
      cur = rows.setdefault(m.group(1), {})
      continue
    m = re.search(r'(ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill|VGPRs|Occupancy \[waves/SIMD\]): (\d+)', line)
    if m and cur is not None:
      cur.setdefault(m.group(1).split(' [')[0], int(m.group(2)))
  hits = [v for k, v in rows.items() if k.startswith(prefix)]
  assert len(hits) == 1, (prefix, len(hits))
  return hits[0]


def test_fixed_shape_class_resources(device_build):
  _, _, log = device_build
  r = _resources(log, FIXED)
  print(r)
  assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['VGPRs'] <= 256 and r['Occupancy'] == 2, r
  assert r['SGPRs Spill'] <= 94, r   # (121 + 67) / 2


def test_generic_instantiations_keep_out_of_scratch(device_build):
  _, _, log = device_build
  for hp in (128, 256, 512):
    for dp in (128, 256):
      r = _resources(log, '_Z11k_decode_rsILi{}ELi{}ELi0ELi0EE'.format(hp, dp))
      print(hp, dp, r)
      assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0, (hp, dp, r)
      assert r['SGPRs Spill'] <= 150, (hp, dp, r)   # 180 .. 194 before, 114 .. 120 with the argument block


def test_step_loop_census(device_build):
  loop_census, asm, _ = device_build
  bodies = loop_census.function_bodies(asm)
  name = [n for n in bodies if n.startswith(FIXED)]
  assert len(name) == 1
  ins, labels = loop_census.instructions(bodies[name[0]])
  span = loop_census.largest_loop(ins, labels)
  c = loop_census.census(ins[span[0]:span[1] + 1])
  print(c)
  assert c['mfma'] == 480, c                                  # the loop that was found IS the step loop
  assert c['v_readlane'] + c['v_writelane'] <= 170, c         # (237 + 102) / 2
  assert c['non-mfma'] <= 4123, c                             # (4260 + 3986) / 2
  assert c['global_load'] == 0, c                             # the frame stream goes through buffer loads
  # the parent commit's own figures (profiles/r07_rs_loop_census.txt): both have to stay below them
  assert c['64-bit address ops'] < 107, c
  assert c['s_nop wait states'] < 569, c
