"""The streaming push's layouts on the host (csrc/uis_push_layout.h): the staging block of a push, the mailbox of a
UIS_FLAG_PERSISTENT session and the rows of the chunk each utterance reads, in tests/push_layout_main.cpp -- built with
the host compiler alone, once plain and once under its sanitizers.  No GPU needed.
"""

import os
import re
import shutil
import subprocess

import pytest

import golden_util
from uisrnn_amd import build as lib_build

ROOT = os.path.normpath(os.path.join(os.path.dirname(golden_util.GOLDEN_DIR), '..'))
CSRC = os.path.join(ROOT, 'uisrnn_amd', 'csrc')
HEADER = 'uis_push_layout.h'
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']


def _compiler():
  cxx = shutil.which(os.environ.get('CXX', '') or 'g++') or shutil.which('c++') or shutil.which('clang++')
  if not cxx:
    pytest.skip('no host C++ compiler')
  return cxx


def _run(cxx, flags, exe):
  subprocess.run([cxx] + flags + ['-I', CSRC, os.path.join(ROOT, 'tests', 'push_layout_main.cpp'), '-o', exe], check=True)
  done = subprocess.run([exe], capture_output=True, text=True)
  assert done.returncode == 0 and done.stdout.startswith('push_layout: ok'), (done.returncode, done.stdout, done.stderr)


def _sources():
  return {name: open(os.path.join(CSRC, name)).read() for name in sorted(os.listdir(CSRC))}


def test_the_header_is_a_dependency_of_the_library():
  assert any(d.endswith(os.path.join('csrc', HEADER)) for d in lib_build.DEPENDS)


def test_the_header_includes_no_hip():
  text = _sources()[HEADER]
  assert 'hip' not in re.sub(r'//.*', '', text).lower()


def test_nothing_is_left_of_what_the_layouts_and_the_chunk_replaced():
  """The fields, the macro and the buffers that the header and the chunk replaced are gone from csrc/."""
  gone = ('pm_o_', 'pm_cluster_rows', 'pm_cap_frames', 'SALLOC', 'chunk_gi0', 'chunk_mse0', 'chunk_bias', 'chunk_hint', 'chunk_pad',
          'h_stage')
  for name, text in _sources().items():
    for word in gone:
      assert word not in text, (name, word)


def test_foff_and_the_bookkeeping_are_written_once():
  """Outside the header nothing forms foff, and `have` advances by the counts in one place."""
  advances = 0
  for name, text in _sources().items():
    if name == HEADER:
      assert text.count('- have[u]') == 1   # the per-cluster fill; the linear one is its case of one cluster
      continue
    assert not re.search(r'-\s*(ss\.)?have\[', text), name
    assert not re.search(r'pos\s*-\s*(ss\.)?have', text), name
    advances += len(re.findall(r'have\[u\]\s*\+=\s*(p\.)?counts\[u\]', text))
  assert advances == 1


def test_the_layouts_plain(tmp_path):
  _run(_compiler(), ['-std=c++17', '-O1', '-g', '-Wall', '-Wextra'], str(tmp_path / 'push_layout'))


def test_the_layouts_under_the_sanitizers(tmp_path):
  cxx = _compiler()
  exe = str(tmp_path / 'push_layout_san')
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
