"""The per-call input tables' host side (csrc/uis_call_tables.h): the rule of every kind of entry point, the setters'
validation, the count checks and the 2^24 bound of a tagged session, in tests/call_tables_main.cpp -- built with the
host compiler alone, once plain and once under its sanitizers.  No GPU needed.
"""

import os
import shutil
import subprocess

import pytest

import golden_util
from uisrnn_amd import build as lib_build

ROOT = os.path.normpath(os.path.join(os.path.dirname(golden_util.GOLDEN_DIR), '..'))
CSRC = os.path.join(ROOT, 'uisrnn_amd', 'csrc')
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']


def _compiler():
  cxx = shutil.which(os.environ.get('CXX', '') or 'g++') or shutil.which('c++') or shutil.which('clang++')
  if not cxx:
    pytest.skip('no host C++ compiler')
  return cxx


def _run(cxx, flags, exe):
  subprocess.run([cxx] + flags + ['-I', CSRC, '-I', os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'call_tables_main.cpp'),
                                  '-o', exe], check=True)
  done = subprocess.run([exe], capture_output=True, text=True)
  assert done.returncode == 0 and done.stdout.startswith('call_tables: ok'), (done.returncode, done.stdout, done.stderr)


def test_the_header_is_a_dependency_of_the_library():
  assert any(d.endswith(os.path.join('csrc', 'uis_call_tables.h')) for d in lib_build.DEPENDS)


def test_no_entry_point_is_left_with_a_rule_of_its_own():
  """The names the header replaced are gone from csrc/, and every opener of a call goes through begin_call."""
  gone = ('take_limits', 'take_bias', 'take_hint', 'take_stream_tags', 'refuse_hint', 'refuse_bias', 'pending_limits',
          'pending_bias3', 'pending_hint', 'pending_stream_tags', 'call_tagged', 'check_bias_frames', 'check_stream_tags_frames')
  openers = 0
  for name in sorted(os.listdir(CSRC)):
    text = open(os.path.join(CSRC, name)).read()
    for word in gone:
      assert word not in text, (name, word)
    openers += text.count('= begin_call(h, "uis_')
  assert openers == 23   # 3 decodes, 2 scores, begin, push, prime, uis_stream_speakers and the 14 other uis_stream_* calls


def test_the_call_tables_plain(tmp_path):
  _run(_compiler(), ['-std=c++17', '-O1', '-g', '-Wall', '-Wextra'], str(tmp_path / 'call_tables'))


def test_the_call_tables_under_the_sanitizers(tmp_path):
  cxx = _compiler()
  exe = str(tmp_path / 'call_tables_san')
  base = ['-std=c++17', '-O1', '-g', '-Wall', '-Wextra'] + SANITIZE
  probe = str(tmp_path / 'probe.cpp')
  with open(probe, 'w') as f:
    f.write('int main() { return 0; }\n')
  # the runtime inside the program where the compiler offers that (the program then starts whatever else the
  # environment loads into it), else the compiler's default
  for flags in (base + ['-static-libasan', '-static-libubsan'], base + ['-static-libsan'], base):
    if subprocess.run([cxx] + flags + [probe, '-o', exe + '_probe'], capture_output=True).returncode == 0:
      break
  else:
    pytest.skip('the host compiler cannot link the sanitizer runtime')
  if subprocess.run([exe + '_probe'], capture_output=True).returncode != 0:
    pytest.skip('a program with the sanitizer runtime does not start in this environment')
  _run(cxx, flags, exe)
