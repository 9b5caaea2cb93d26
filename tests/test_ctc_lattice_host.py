"""The host-usable half of csrc/ctc_lattice.h (states-per-lane dispatch list, state predicates, refusal rule, row map) checked
exhaustively against direct restatements of the definitions, without a GPU: tests/host_cpp/ctc_lattice_check.cpp, built from the
header alone with the host compiler -- once plainly and once as a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('flags', [[], ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']], ids=['plain', 'sanitized'])
def test_ctc_lattice_on_host(tmp_path, flags):
  exe = str(tmp_path / 'ctc_lattice_check')
  subprocess.check_call(['g++', '-O1', '-g', '-std=c++17'] + flags +
                        ['-I' + os.path.join(ROOT, 'speecht_amd', 'csrc'), '-I' + os.path.join(ROOT, 'include'),
                         os.path.join(ROOT, 'tests', 'host_cpp', 'ctc_lattice_check.cpp'), '-o', exe])
  r = subprocess.run([exe], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  assert 'checked lattice_kpl for L = -1..512 and 303 label strings' in r.stdout, r.stdout
