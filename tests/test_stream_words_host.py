"""The host forms of the ring alignment and the ring confidences (st_ctc_align_ring_host, st_ctc_word_conf_ring_host,
csrc/stream_words.hip, csrc/stream_ring.h) as a stand-alone program with its own main, tests/host_cpp/stream_words_host_check.cpp,
whose host code is built under the address and undefined-behaviour sanitizers: a ring filled by the keep rule from streams that wrap
it several times, jobs starting at every ring offset held bit for bit to the dense host forms, a job of exactly max_rows rows, jobs
of 0 rows and the jobs the ring cannot serve.  Needs no GPU."""
import os
import subprocess

from speecht_amd.build import HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ring_host_forms_under_sanitizers(tmp_path):
  exe = str(tmp_path / 'stream_words_host_check')
  csrc = os.path.join(ROOT, 'speecht_amd', 'csrc')
  san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
  subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O1', '-g', '-std=c++17', '-w'] + [f for s in san for f in ('-Xarch_host', s)] +
                        ['-I' + csrc, '-I' + os.path.join(ROOT, 'include')] +
                        [os.path.join(csrc, f) for f in ('stream_words.hip', 'ctc_align.hip', 'ctc_conf.hip', 'api.hip')] +
                        [os.path.join(ROOT, 'tests', 'host_cpp', 'stream_words_host_check.cpp'), '-o', exe, san[0]])
  r = subprocess.run([exe], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  assert 'starting at all 14 ring offsets, the ring wrapped 9 times' in r.stdout, r.stdout
  assert 'checked jobs of 0 rows and the jobs the ring cannot serve' in r.stdout and 'checked the refusals' in r.stdout, r.stdout
