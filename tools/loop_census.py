#!/usr/bin/env python3
"""Static instruction census of a decode kernel's step loop, without a GPU.

  python tools/loop_census.py [--kernel 'k_decode_rs<512, 256, 10, 16>'] [--out FILE] [--asm FILE] [-D NAME ...]

Compiles the decoder's device code for gfx950 to assembly with the library's own flags, finds the
named instantiation, takes the largest backward-branch span of its body (the step loop: every stage
of a decode step, all row-count variants of the dense stages included) and counts what the
instruction-bound stretches of the step are made of.  A static count: it says nothing about how
often a path runs, only what the compiler emitted -- spill shuttles (v_readlane / v_writelane and
the s_nop wait states behind them), 64-bit address arithmetic per lane, loads by flavour.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uisrnn_amd import build as hip_build  # noqa: E402

ADDR64 = ('v_mad_u64_u32', 'v_mad_i64_i32', 'v_addc_co_u32', 'v_lshl_add_u64', 'v_lshlrev_b64')


def compile_asm(defines, path):
  flags = [f for f in hip_build.FLAGS if f not in ('-shared', '-fPIC')]
  cmd = [hip_build.hipcc()] + flags + ['--cuda-device-only', '-S'] + ['-D' + d for d in defines] + \
        ['-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'uisrnn_amd', 'csrc'),
         hip_build.SOURCES[0], '-o', path]
  subprocess.run(cmd, check=True)


def mangled_prefix(kernel):
  """'k_decode_rs<512, 256, 10, 16>' -> '_Z11k_decode_rsILi512ELi256ELi10ELi16EE' (integer and bool arguments; no demangler needed)."""
  if kernel.startswith('_Z'):
    return kernel
  m = re.match(r'^\s*(\w+)\s*(?:<(.*)>)?\s*$', kernel)
  if not m:
    sys.exit('cannot read the kernel name ' + repr(kernel))
  out = '_Z{}{}'.format(len(m.group(1)), m.group(1))
  if m.group(2) is not None:
    out += 'I'
    for a in m.group(2).split(','):
      a = a.strip()
      out += {'true': 'Lb1E', 'false': 'Lb0E'}.get(a) or 'Li{}E'.format(a.replace('-', 'n'))
    out += 'E'
  return out


def function_bodies(text):
  """{mangled name: [lines]} of every global function of the assembly file."""
  bodies, cur, name = {}, None, None
  for line in text.splitlines():
    m = re.match(r'^(_Z\w+):', line)
    if m and cur is None:
      name, cur = m.group(1), []
      continue
    if cur is not None:
      if re.match(r'^\.Lfunc_end\d+:', line):
        bodies[name] = cur
        cur = None
      else:
        cur.append(line)
  return bodies


def instructions(lines):
  """[(mnemonic, operands)] and {label: index of the next instruction}."""
  ins, labels = [], {}
  for line in lines:
    s = line.split(';')[0].strip()
    if not s:
      continue
    m = re.match(r'^(\.LBB\d+_\d+):', s)
    if m:
      labels[m.group(1)] = len(ins)
      continue
    if s.startswith('.') or s.endswith(':'):
      continue
    parts = s.split(None, 1)
    ins.append((parts[0], parts[1] if len(parts) > 1 else ''))
  return ins, labels


def largest_loop(ins, labels):
  best = None
  for i, (op, args) in enumerate(ins):
    if op.startswith('s_cbranch') or op == 's_branch':
      tgt = labels.get(args.strip())
      if tgt is not None and tgt <= i and (best is None or i - tgt > best[1] - best[0]):
        best = (tgt, i)
  return best


def census(ins):
  c = {}
  def count(pred):
    return sum(1 for op, _ in ins if pred(op))
  c['total'] = len(ins)
  c['mfma'] = count(lambda o: o.startswith('v_mfma'))
  c['non-mfma'] = c['total'] - c['mfma']
  c['v_readlane'] = count(lambda o: o.startswith('v_readlane'))
  c['v_writelane'] = count(lambda o: o.startswith('v_writelane'))
  c['s_nop'] = count(lambda o: o == 's_nop')
  c['s_nop wait states'] = sum(int(a.strip(), 0) + 1 for o, a in ins if o == 's_nop')
  c['s_waitcnt'] = count(lambda o: o.startswith('s_waitcnt'))
  for name in ADDR64:
    c[name] = count(lambda o, n=name: o.startswith(n))
  c['64-bit address ops'] = sum(c[n] for n in ADDR64)
  c['global_load'] = count(lambda o: o.startswith('global_load'))
  c['global_store'] = count(lambda o: o.startswith('global_store') or o.startswith('global_atomic'))
  c['buffer_load'] = count(lambda o: o.startswith('buffer_load'))
  c['buffer_store'] = count(lambda o: o.startswith('buffer_store'))
  c['s_load'] = count(lambda o: o.startswith('s_load'))
  c['ds_read'] = count(lambda o: o.startswith('ds_read') or o.startswith('ds_load'))
  c['ds_write'] = count(lambda o: o.startswith('ds_write') or o.startswith('ds_store'))
  c['s_barrier'] = count(lambda o: o == 's_barrier')
  return c


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--kernel', default='k_decode_rs<512, 256, 10, 16>',
                  help='demangled name (up to the argument list) of the instantiation')
  ap.add_argument('--asm', default=None, help='count an existing assembly file instead of compiling')
  ap.add_argument('--out', default=None, help='append the table to this file')
  ap.add_argument('--label', default='', help='a heading for the table (which build this is)')
  ap.add_argument('-D', dest='defines', action='append', default=[])
  args = ap.parse_args()
  if args.asm:
    text = open(args.asm).read()
  else:
    with tempfile.TemporaryDirectory() as tmp:
      path = os.path.join(tmp, 'decoder.s')
      compile_asm(args.defines, path)
      text = open(path).read()
  bodies = function_bodies(text)
  want = mangled_prefix(args.kernel)
  hits = [n for n in bodies if n.startswith(want)]
  if len(hits) != 1:
    sys.exit('{} functions start with {} ({!r}); the file has: {}'.format(len(hits), want, args.kernel, ', '.join(sorted(bodies))))
  ins, labels = instructions(bodies[hits[0]])
  span = largest_loop(ins, labels)
  if span is None:
    sys.exit('no backward branch in ' + hits[0])
  loop = ins[span[0]:span[1] + 1]
  c = census(loop)
  out = ['# {}{}'.format(args.kernel, ' -- ' + args.label if args.label else ''),
         '# largest backward-branch span: instructions {} .. {} of {} in the kernel'.format(span[0], span[1], len(ins))]
  out += ['{:<22} {:>6}'.format(k, v) for k, v in c.items()]
  text_out = '\n'.join(out) + '\n'
  sys.stdout.write(text_out)
  if args.out:
    with open(args.out, 'a') as f:
      f.write(text_out + '\n')


if __name__ == '__main__':
  main()
