"""The host form of following a script in live streams (st_ctc_follow_stream_host, csrc/ctc_follow_stream.hip) as a stand-alone
program with its own main, tests/host_cpp/ctc_follow_host_check.cpp, whose host code is built under the address and
undefined-behaviour sanitizers: the sizes, bad arguments, a planted script, a buffer of one event, a script longer than the state
and a script of 1 000 ids across three state blocks in uneven steps.  Needs no GPU."""
import os
import subprocess

from speecht_amd.build import HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_follow_host_form_under_sanitizers(tmp_path):
  exe = str(tmp_path / 'ctc_follow_host_check')
  csrc = os.path.join(ROOT, 'speecht_amd', 'csrc')
  san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
  subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O1', '-g', '-std=c++17', '-w'] + [f for s in san for f in ('-Xarch_host', s)] +
                        ['-I' + csrc, '-I' + os.path.join(ROOT, 'include'), os.path.join(csrc, 'ctc_follow_stream.hip'),
                         os.path.join(csrc, 'api.hip'), os.path.join(ROOT, 'tests', 'host_cpp', 'ctc_follow_host_check.cpp'), '-o', exe,
                         san[0]])
  r = subprocess.run([exe], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  assert 'checked a script of 1000 ids on 1300 frames in uneven steps' in r.stdout, r.stdout
