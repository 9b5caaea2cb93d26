"""The host forms of the waveform augmentation (st_wave_augment_host, st_wave_augment_plan_host; csrc/wave_augment.hip) as a
stand-alone program with its own main, tests/host_cpp/wave_augment_host_check.cpp, whose host code is built under the address and
undefined-behaviour sanitizers: the edge lengths at six speeds and the three-speed policy, with and without a noise bank, into
buffers with not one float to spare, and bad arguments.  Needs no GPU."""
import os
import subprocess

from speecht_amd.build import HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wave_augment_host_forms_under_sanitizers(tmp_path):
  exe = str(tmp_path / 'wave_augment_host_check')
  csrc = os.path.join(ROOT, 'speecht_amd', 'csrc')
  san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
  subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O1', '-g', '-std=c++17', '-w'] + [f for s in san for f in ('-Xarch_host', s)] +
                        ['-I' + csrc, '-I' + os.path.join(ROOT, 'include'), os.path.join(csrc, 'wave_augment.hip'),
                         os.path.join(csrc, 'api.hip'), os.path.join(ROOT, 'tests', 'host_cpp', 'wave_augment_host_check.cpp'), '-o', exe,
                         san[0]])
  r = subprocess.run([exe], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  assert 'replaced plans over the edge lengths' in r.stdout, r.stdout
