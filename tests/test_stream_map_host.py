"""The index arithmetic of streaming recognition (csrc/stream_map.h) as a stand-alone program with its own main,
tests/host_cpp/stream_map_check.cpp, built under the address and undefined-behaviour sanitizers: ready outputs and retained
frames against an enumeration of receptive fields, then whole streams through the eleven layers in chunks.  Needs no GPU."""
import os
import subprocess

from speecht_amd.build import HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_map_on_host_under_sanitizers(tmp_path):
  exe = str(tmp_path / 'stream_map_check')
  csrc = os.path.join(ROOT, 'speecht_amd', 'csrc')
  san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
  subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-x', 'hip', '-O1', '-g', '-std=c++17', '-w'] +
                        [f for s in san for f in ('-Xarch_host', s)] +
                        ['-I' + csrc, os.path.join(ROOT, 'tests', 'host_cpp', 'stream_map_check.cpp'), '-o', exe, san[0]])
  r = subprocess.run([exe], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  assert 'checked 1040 streams; first logits row after 99 input frames' in r.stdout, r.stdout
