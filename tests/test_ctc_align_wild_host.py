"""The host forms of the wildcard aligners (st_ctc_align_wild_host, csrc/ctc_align.hip; st_ctc_align_long_wild_host,
csrc/ctc_align_long.hip) as a stand-alone program with its own main, tests/host_cpp/ctc_align_wild_host_check.cpp, whose host code
is built under the address and undefined-behaviour sanitizers: small cases, a wildcard at each end, bad arguments and one label of
600 ids across two state blocks with a wildcard on the block edge.  Needs no GPU."""
import os
import subprocess

from speecht_amd.build import HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_align_wild_host_forms_under_sanitizers(tmp_path):
  exe = str(tmp_path / 'ctc_align_wild_host_check')
  csrc = os.path.join(ROOT, 'speecht_amd', 'csrc')
  san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
  subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O1', '-g', '-std=c++17', '-w'] + [f for s in san for f in ('-Xarch_host', s)] +
                        ['-I' + csrc, '-I' + os.path.join(ROOT, 'include'), os.path.join(csrc, 'ctc_align.hip'),
                         os.path.join(csrc, 'ctc_align_long.hip'), os.path.join(csrc, 'api.hip'),
                         os.path.join(ROOT, 'tests', 'host_cpp', 'ctc_align_wild_host_check.cpp'), '-o', exe, san[0]])
  r = subprocess.run([exe], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  assert 'checked a label of 600 ids across two state blocks with a wildcard on the block edge' in r.stdout, r.stdout
