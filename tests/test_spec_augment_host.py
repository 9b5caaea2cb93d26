"""The host form of SpecAugment (st_spec_augment_host / st_spec_augment_plan_host, csrc/spec_augment.hip) as a stand-alone program
with its own main, tests/host_cpp/spec_augment_host_check.cpp, whose host code is built under the address and undefined-behaviour
sanitizers: the lengths around the warp's threshold, 13 channels, one frame, one utterance, masks wider than the utterance, bad
arguments, into buffers with nothing to spare.  Needs no GPU; the program runs as a plain child process."""
import os
import subprocess

from speecht_amd.build import HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spec_augment_host_form_under_sanitizers(tmp_path):
  exe = str(tmp_path / 'spec_augment_host_check')
  csrc = os.path.join(ROOT, 'speecht_amd', 'csrc')
  san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
  subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O1', '-g', '-std=c++17', '-w'] + [f for s in san for f in ('-Xarch_host', s)] +
                        ['-I' + csrc, '-I' + os.path.join(ROOT, 'include'), os.path.join(csrc, 'spec_augment.hip'), os.path.join(csrc, 'api.hip'),
                         os.path.join(ROOT, 'tests', 'host_cpp', 'spec_augment_host_check.cpp'), '-o', exe, san[0]])
  r = subprocess.run([exe], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  assert 'checked 72 batches through the host form' in r.stdout, r.stdout
