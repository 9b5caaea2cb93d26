"""The host side of keyword spotting in live streams (st_ctc_spot_stream_plan, st_ctc_spot_stream_host, csrc/ctc_spot_stream.hip) as
a stand-alone program with its own main, tests/host_cpp/ctc_spot_stream_host_check.cpp, whose host code is built under the address
and undefined-behaviour sanitizers: the packed layouts, bad arguments, streams fed in steps under both packings and the longest
keyword the lattice holds.  Needs no GPU."""
import os
import subprocess

from speecht_amd.build import HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spot_stream_host_form_under_sanitizers(tmp_path):
  exe = str(tmp_path / 'ctc_spot_stream_host_check')
  csrc = os.path.join(ROOT, 'speecht_amd', 'csrc')
  san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
  subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O1', '-g', '-std=c++17', '-w'] + [f for s in san for f in ('-Xarch_host', s)] +
                        ['-I' + csrc, '-I' + os.path.join(ROOT, 'include'), os.path.join(csrc, 'ctc_spot_stream.hip'),
                         os.path.join(csrc, 'api.hip'), os.path.join(ROOT, 'tests', 'host_cpp', 'ctc_spot_stream_host_check.cpp'), '-o', exe,
                         san[0]])
  r = subprocess.run([exe], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  assert 'checked a keyword of 511 ids on 700 frames in uneven steps' in r.stdout, r.stdout
