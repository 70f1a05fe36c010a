"""k_decode_rs's second instruction diet (LABNOTES R8.1), checked without a GPU, beside test_rs_loop_static.py: the step loop
of the fixed-shape class after the row counts became one 64-bit word (a wave's first row and the step's total are byte
sums: no per-slot conditions kept, and spilled, across the loop), the statistics one 16-byte update per step, the debug
array's address a load behind its flag, the frame rows 32-bit.

The bounds lie half way between the parent commit's census and this change's (tools/loop_census.py and
tools/resource_table.py on both; profiles/r08_rs_loop_census.txt, profiles/r08_kernel_resources.txt), so that a change
that brings the old state back fails here and a compiler update has room:

                                  parent    now    bound
  loop: non-MFMA instructions       3988   3935     3961
  loop: v_readlane                   104     85       94
  spilled SGPRs                       70     55       62
  loop: s_barrier                     15     15       15   (the row list keeps its two barriers: LABNOTES R8.1)
"""

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
  tmp = tmp_path_factory.mktemp('census_r8')
  asm = str(tmp / 'decoder.s')
  flags = [f for f in hip_build.FLAGS if f not in ('-shared', '-fPIC')]
  cmd = [hip_build.hipcc()] + flags + ['--cuda-device-only', '-S', '-Rpass-analysis=kernel-resource-usage',
                                       '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'uisrnn_amd', 'csrc'),
                                       hip_build.SOURCES[0], '-o', asm]
  log = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode()
  return loop_census, open(asm).read(), log


def _resources(log):
  rows, cur = {}, None
  for line in log.splitlines():
    m = re.search(r'Function Name: (\S+)', line)
    if m:
      cur = rows.setdefault(m.group(1), {})
      continue
    m = re.search(r'(ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill|VGPRs|Occupancy \[waves/SIMD\]): (\d+)', line)
    if m and cur is not None:
      cur.setdefault(m.group(1).split(' [')[0], int(m.group(2)))
  return rows


def test_fixed_shape_class_loop_and_spills(device_build):
  loop_census, asm, log = device_build
  bodies = loop_census.function_bodies(asm)
  name = [n for n in bodies if n.startswith(FIXED)]
  assert len(name) == 1
  ins, labels = loop_census.instructions(bodies[name[0]])
  span = loop_census.largest_loop(ins, labels)
  c = loop_census.census(ins[span[0]:span[1] + 1])
  print(c)
  assert c['mfma'] == 480, c              # the loop that was found IS the step loop
  assert c['non-mfma'] <= 3961, c         # (3988 + 3935) / 2
  assert c['v_readlane'] <= 94, c         # (104 + 85) / 2
  assert c['s_barrier'] <= 15, c          # 15 before and after
  r = [v for k, v in _resources(log).items() if k.startswith(FIXED)]
  assert len(r) == 1
  print(r[0])
  assert r[0]['SGPRs Spill'] <= 62, r[0]  # (70 + 55) / 2
  assert r[0]['ScratchSize'] == 0 and r[0]['VGPRs Spill'] == 0 and r[0]['VGPRs'] <= 256 and r[0]['Occupancy'] == 2, r[0]


def test_generic_and_limit_twins_stay_out_of_scratch(device_build):
  _, _, log = device_build
  rows = {k: v for k, v in _resources(log).items() if k.startswith('_Z11k_decode_rsI')}
  assert len(rows) >= 14, sorted(rows)    # six generic shapes and the fixed-shape class, each with its twin for limits
  for k, v in rows.items():
    print(k, v)
    assert v['ScratchSize'] == 0 and v['VGPRs Spill'] == 0, (k, v)
