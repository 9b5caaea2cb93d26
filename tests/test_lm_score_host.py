"""The host form of the sentence scores (st_lm_score_prefixes_host, csrc/lm_score.hip) as a stand-alone program with its own main,
tests/host_cpp/lm_score_host_check.cpp, whose host code is built under the address and undefined-behaviour sanitizers: no
prefixes, a pitch above every length, bad ids, the longest prefix, and models of orders 1 and 5.  Needs no GPU."""
import os
import subprocess

from speecht_amd.build import HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sentence_score_host_form_under_sanitizers(tmp_path):
  exe = str(tmp_path / 'lm_score_host_check')
  csrc = os.path.join(ROOT, 'speecht_amd', 'csrc')
  san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
  subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O1', '-g', '-std=c++17', '-w'] + [f for s in san for f in ('-Xarch_host', s)] +
                        ['-I' + csrc, '-I' + os.path.join(ROOT, 'include'), os.path.join(csrc, 'lm_score.hip'), os.path.join(csrc, 'lm.hip'),
                         os.path.join(csrc, 'api.hip'), os.path.join(ROOT, 'tests', 'host_cpp', 'lm_score_host_check.cpp'), '-o', exe, san[0]])
  r = subprocess.run([exe], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  assert 'checked a prefix of 1501 ids at orders 1 and 5' in r.stdout, r.stdout
