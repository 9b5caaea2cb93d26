"""The host form of the endpointer (st_stream_endpoint_host, the walk of csrc/stream_endpoint_core.h the kernel shares) against the
specification, tests/endpoint_oracle.py: events, pieces, ids and the carried state of every step, for every way of cutting the rows
into steps; then the same sweep as a stand-alone program with its own main, tests/host_cpp/stream_endpoint_check.cpp, under the
address and undefined-behaviour sanitizers.  Needs no GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import endpoint_cases as EC
from tests import endpoint_oracle as EO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
  from speecht_amd import _lib
  return _lib.load()


def test_entry_points_are_exported_and_sized(lib):
  from speecht_amd import _lib
  for name in ('st_stream_endpoint_state_bytes', 'st_stream_endpoint_score_bytes', 'st_stream_endpoint_pieces', 'st_ctc_greedy_endpoint_stream', 'st_stream_endpoint_host',
               'st_ctc_beam_stream_step_pieces'):
    assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
  assert lib.st_stream_endpoint_state_bytes() == 32 and lib.st_stream_endpoint_score_bytes() == 1024
  for n in (1, 2, 7, 13, 83, 500):
    for R, L, M in EC.PARAMS + [(25, 50, 1500)]:
      assert lib.st_stream_endpoint_pieces(n, R, L, M) == EO.pieces_needed(n, R, L, M)
  for bad in ((0, 1, 1, 1), (5, 0, 1, 1), (5, 1, 0, 1), (5, 1, 3, 2)):
    assert lib.st_stream_endpoint_pieces(*bad) == 0


def test_host_form_equals_the_specification_for_every_cut(lib):
  total = {}
  for seed, S, C, space_id, R, L, M in EC.sweep():
    logits, lens = EC.make_streams(seed, S, C, space_id, R, L, M)
    plans = EC.cut_plans(S)
    for i in [(seed + j) % len(plans) for j in (0, 2, 5)]:          # three of the seven cuts per case, every cut across the sweep
      cuts = plans[i]
      seen, _, _ = EC.drive(EC.host_step_fn(lib, C, space_id, R, L, M, S), logits, lens, C, space_id, R, L, M, cuts,
                            sit_out=i % 2 == 0, finish_apart=(0,) if i % 3 == 0 else ())
      for key, n in seen.items():
        total[key] = total.get(key, 0) + n
  assert all(total[kind] > 100 for kind in (1, 2, 3, 4)), total
  assert all(total[name] > 20 for name in EC.SITUATIONS), total


def test_ties_are_speech_or_silent_as_the_greedy_decoder_reads_them(lib):
  C, space = 5, 3
  x = np.full((6, EC.PITCH), EC.POISON, np.float32)
  x[:, :C] = 0.0
  x[0, [1, 4]] = 2.0                                                # blank = label: the label wins -> speech
  x[1, [3, 4]] = 2.0                                                # space = blank: silent
  x[2, 4] = 2.0                                                     # blank
  x[3, 3] = 2.0                                                     # space
  x[4, [0, 3]] = 2.0                                                # label = space: the label wins -> speech
  x[5, :C] = 1.0                                                    # all equal: class 0 -> speech
  assert EO.silent_rows(x, C, space).tolist() == [False, True, True, True, False, False]
  assert EO.silent_rows(x, C, -1).tolist() == [False, False, True, False, False, False]
  for space_id, want in ((space, [(1, 0, 4, 0, 0, 0)]), (-1, [])):
    step = EC.host_step_fn(lib, C, space_id, 3, 4, 40, 1)
    out = step(x, np.asarray([(0, t) for t in range(6)], np.int32), np.asarray([[0, 6, -1, 1]], np.int32), 6, EO.pieces_needed(6, 3, 4, 40))
    got = [tuple(e[:5].tolist()) + (int(e[7]),) for e in out.events[0][:[int(e[0]) for e in out.events[0]].index(0)]]
    assert got == want and got == EO.Spec(x, C, space_id, 3, 4, 40).row_events


def test_bad_requests_are_refused(lib):
  S, P = 1, 4
  buf, rows, table = np.zeros((4, 32), np.float32), np.zeros((4, 2), np.int32), np.asarray([[0, 4, -1, 1]], np.int32)
  state, score, ids, count, neg = np.zeros(8, np.int32), np.zeros(256, np.float32), np.zeros(8, np.int32), np.zeros(1, np.int32), np.zeros(1, np.float32)
  events, pieces = np.zeros(P * 8, np.int32), np.zeros(P * 4, np.int32)
  p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
  ok = dict(C=29, space=27, R=2, L=3, M=9, max_rows=4, max_new=8, P=P, events=p(events))

  def run(**kw):
    a = dict(ok, **kw)
    return lib.st_stream_endpoint_host(p(buf), 32, a['C'], p(rows), p(table), S, a['space'], a['R'], a['L'], a['M'], a['max_rows'], p(state),
                                       p(score), p(ids), a['max_new'], p(count), p(neg), a['events'], p(pieces), a['P'])

  assert run() == 0
  for kw, text in ((dict(R=0), 'silence_frames'), (dict(L=0), 'lead_frames'), (dict(M=2), 'below lead_frames'), (dict(space=29), 'space_id'),
                   (dict(space=-2), 'space_id'), (dict(P=2), 'pieces'), (dict(max_rows=0), 'max_rows'), (dict(C=1), 'classes'),
                   (dict(C=65), 'classes'), (dict(events=None), 'null'), (dict(max_new=0), 'positive')):
    assert run(**kw) != 0, kw
    assert text in lib.st_last_error().decode(), (kw, lib.st_last_error().decode())


def test_endpoint_walk_on_host_under_sanitizers(tmp_path):
  from speecht_amd.build import HIPCC
  exe = str(tmp_path / 'stream_endpoint_check')
  csrc = os.path.join(ROOT, 'speecht_amd', 'csrc')
  san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
  subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-x', 'hip', '-O1', '-g', '-std=c++17', '-w'] +
                        [f for s in san for f in ('-Xarch_host', s)] +
                        ['-I' + csrc, os.path.join(ROOT, 'tests', 'host_cpp', 'stream_endpoint_check.cpp'), '-o', exe, san[0]])
  r = subprocess.run([exe], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  assert 'streams; events 1/2/3/4:' in r.stdout and 'all cuts agree' in r.stdout, r.stdout
