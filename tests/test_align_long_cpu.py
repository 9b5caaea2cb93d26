"""Tiled forced alignment without a GPU: the host form st_ctc_align_long_host (plain loops over the whole lattice, the
arithmetic of csrc/ctc_align_core.h, the back-pointer layout of the device) against st_ctc_align_host on labels that one takes,
against the float64 oracle (tests/align_oracle.py) beyond them, the workspace formula and the argument validation of both entry
points, the CLI surface of `speecht-cli align --segment`, and `alignment.concat_frame_seconds`.

Accuracy condition: that of tests/test_align_cpu.py.  The lattice is kept in double, so the path is the float64 optimum (its
loss against the oracle's score is the rounding of two summation orders) and the score, returned as a double, is far inside."""
import ctypes
import importlib.machinery
import importlib.util
import os

import numpy as np
import pytest

from tests import align_oracle as AO
from tests.align_long_util import _p, edge_labels, host_align_long, states_from_spans, workspace_bytes
from tests.test_align_cpu import host_align

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_EINVAL = -1


def _cli():
  loader = importlib.machinery.SourceFileLoader('speecht_cli_align_long', os.path.join(ROOT, 'speecht-cli'))
  spec = importlib.util.spec_from_loader('speecht_cli_align_long', loader)
  cli = importlib.util.module_from_spec(spec)
  loader.exec_module(cli)
  return cli


def test_library_exports_the_long_aligner_and_the_constants():
  from speecht_amd import _lib, engine_decode as ED
  lib = _lib.load()
  for name in ('st_ctc_align_long_ws', 'st_ctc_align_long_f32', 'st_ctc_align_long_host'):
    assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS
  assert (ED.ALIGN_LONG_FRAME_BLOCK, ED.ALIGN_LONG_STATE_BLOCK, ED.MAX_ALIGN_LONG_LABELS) == (64, 896, 1048575)
  assert ED.MAX_ALIGN_LABELS == 511


def test_host_form_equals_the_one_wave_host_form():
  """Labels of 0 .. 511 ids, ragged frame counts, repeats, labels that do not fit, 2 .. 32 classes, a row pitch above the classes."""
  rng = np.random.default_rng(31)
  cases = [(0, 1), (0, 9), (1, 1), (1, 2), (511, 700), (511, 1023), (40, 30)]
  for _ in range(60):
    T = int(rng.integers(1, 300))
    cases.append((int(rng.integers(0, T // 2 + 2)), T))
  fits = 0
  for n, (L, T) in enumerate(cases):
    C = int(rng.choice([2, 3, 5, 17, 29, 32]))
    lab = AO.random_labels(rng, L, C, repeat_prob=float(rng.choice([0.0, 0.3])))
    if n >= 7 and n % 3 == 0:
      T = max(AO.min_frames(lab) + int(rng.integers(-1, 2)), 1)             # around the edge of fitting
    x = AO.random_logits(rng, T, C, scale=float(rng.choice([0.05, 1.0, 3.0, 10.0])))
    padded = np.full((T, C + 3), 1e30, dtype=np.float32)
    padded[:, :C] = x
    spans, score, status = host_align_long(padded, lab, classes=C, fill=0xFF)
    s0, _, sc0, st0 = host_align(x[None], [lab], [T])
    assert status == st0[0] == int(T < AO.min_frames(lab)), (L, T)
    assert (spans == s0[0]).all() and np.float32(score) == sc0[0], (L, T)
    if status:
      assert score == -np.inf and (spans == -1).all()
    fits += status == 0
  assert 40 <= fits < len(cases)


@pytest.mark.parametrize('L,T', [(512, 1100), (896, 2000), (1400, 3000)])
def test_host_form_against_the_oracle(L, T):
  rng = np.random.default_rng(L)
  C = 29
  lab = edge_labels(rng, L, C)
  T = max(T, AO.min_frames(lab))
  x = AO.random_logits(rng, T, C)
  ref = AO.align64(x, lab)
  spans, score, status = host_align_long(x, lab)
  states = states_from_spans(spans, T)
  assert status == 0 and AO.is_valid_alignment(states, lab)
  assert (spans[:, 0] < spans[:, 1]).all() and (spans[1:, 0] >= spans[:-1, 1]).all()
  r = AO.accuracy_ratios(x, lab, states, score, ref[2])
  print('host form, T = {}, L = {}: ratios to the accuracy bounds: path {:.3g}, score {:.3g}'.format(T, L, *r))
  assert r[0] <= 1.0 and r[1] <= 1.0
  # all-zero logits: every comparison is an exact tie, the tie rule alone decides; planted logits: one clear path
  zero = np.zeros((T, C), dtype=np.float32)
  assert (host_align_long(zero, lab)[0] == AO.align64(zero, lab)[1]).all()
  xp, path = AO.planted_logits(rng, lab, T, C)
  sp, sc, st = host_align_long(xp, lab, fill=0xFF)
  assert st == 0 and (sp == AO.align64(xp, lab)[1]).all()
  assert list(states_from_spans(sp, T)) == [u // 2 if u & 1 else -1 for u in path]


def test_host_form_forced_diagonal():
  L = 2000
  lab = [(5 * k) % 28 for k in range(L)]
  x = AO.random_logits(np.random.default_rng(5), L, 29)
  spans, score, status = host_align_long(x, lab)
  assert status == 0 and (spans == np.stack([np.arange(L), np.arange(L) + 1], axis=1)).all()
  assert host_align_long(x[:-1], lab)[2] == 1


def test_workspace_formula_and_argument_validation():
  from speecht_amd import _lib
  lib = _lib.load()
  for T, L in ((1, 0), (10, 3), (1000, 447), (1000, 448), (70, 895), (70, 896), (3000, 1400), (248000, 54000), (5, 1048575)):
    nb = (2 * L + 1 + 895) // 896
    assert lib.st_ctc_align_long_ws(T, L) == T * (32 * 8 + 56 * 4 * nb) + 2 * (896 * nb + 128) * 8 + 512 == workspace_bytes(T, L)
  assert lib.st_ctc_align_long_ws(0, 3) == 0 and lib.st_ctc_align_long_ws(-5, 3) == 0
  assert lib.st_ctc_align_long_ws(10, -1) == 0 and lib.st_ctc_align_long_ws(10, 1048576) == 0
  T, C, L = 10, 5, 2
  x = np.zeros((T, 32), dtype=np.float32)
  ids = np.zeros(4, dtype=np.int32)
  spans, score, status = np.zeros((4, 2), dtype=np.int32), np.zeros(1), np.zeros(1, dtype=np.int32)
  need = lib.st_ctc_align_long_ws(T, L)
  ws = np.zeros(need // 8 + 2, dtype=np.float64)

  def host(**kw):
    a = dict(logits=_p(x), T=T, C=C, pitch=32, ids=_p(ids), L=L, spans=_p(spans), score=_p(score), status=_p(status), ws=_p(ws),
             nbytes=ws.nbytes)
    a.update(kw)
    return lib.st_ctc_align_long_host(a['logits'], a['T'], a['C'], a['pitch'], a['ids'], a['L'], a['spans'], a['score'], a['status'],
                                      a['ws'], a['nbytes'])

  def device(**kw):
    # every argument is refused before anything is launched: no device is touched
    a = dict(logits=_p(x), T=T, C=C, pitch=32, ids=_p(ids), L=L, spans=_p(spans), score=_p(score), status=_p(status), ws=_p(ws),
             nbytes=ws.nbytes)
    a.update(kw)
    return lib.st_ctc_align_long_f32(a['logits'], a['T'], a['C'], a['pitch'], a['ids'], a['L'], a['spans'], a['score'], a['status'],
                                     a['ws'], a['nbytes'], None)

  assert host() == 0
  assert host(L=0, ids=None) == 0                      # an empty label needs no ids
  for fn in (host, device):
    for name in ('logits', 'ids', 'spans', 'score', 'status', 'ws'):
      assert fn(**{name: None}) == ST_EINVAL, (fn.__name__, name)
      assert b'null' in lib.st_last_error()
    assert fn(L=-1) == ST_EINVAL and fn(L=1048576) == ST_EINVAL and b'1048575' in lib.st_last_error()
    assert fn(T=0) == ST_EINVAL and fn(T=-3) == ST_EINVAL
    assert fn(nbytes=need - 1) == ST_EINVAL and b'workspace' in lib.st_last_error()
    assert fn(ws=ctypes.c_void_p(ws.ctypes.data + 8)) == ST_EINVAL and b'aligned' in lib.st_last_error()
    assert fn(C=33, pitch=64) == ST_EINVAL and b'num_classes' in lib.st_last_error()
    assert fn(C=1) == ST_EINVAL and fn(C=5, pitch=4) == ST_EINVAL


def test_cli_align_segment_parses(capsys):
  cli = _cli()
  from speecht_amd import alignment, segmentation
  _, flags = cli.parse(['align', 'a.wav'])
  assert not hasattr(flags, 'segment') and not hasattr(flags, 'confidence') and alignment.segment_options(flags) is None
  _, flags = cli.parse(['align', '--segment', '--batch-size', '4', '--mask-padding', 'a.wav'])
  assert flags.segment and flags.batch_size == 4 and flags.mask_padding
  # the defaults of `transcribe --segment`
  _, tr = cli.parse(['transcribe', '--segment', 'a.wav'])
  assert alignment.segment_options(flags) == segmentation.SegmentOptions() == segmentation.SegmentOptions(
      threshold=tr.segment_threshold, min_silence=tr.min_silence, max_segment=tr.max_segment)
  _, flags = cli.parse(['align', '--segment', '--segment-threshold', '0.05', '--min-silence', '0.5', '--max-segment', '12', 'a.wav'])
  assert alignment.segment_options(flags) == segmentation.SegmentOptions(threshold=0.05, min_silence=0.5, max_segment=12.0)
  assert cli.parse(['align', '--confidence', 'a.wav'])[1].confidence
  with pytest.raises(SystemExit) as e:
    cli.parse(['align', '--segment', '--confidence', 'a.wav'])
  assert e.value.code == 2 and '--confidence is not available with --segment' in capsys.readouterr().err


def test_without_segment_a_long_transcript_is_still_too_long():
  from speecht_amd import alignment
  golden = os.path.join(ROOT, 'tests', 'golden', '1089-134686-0037.flac')
  r, = alignment.align_files(None, [golden], ['A' * 512])
  assert r['error'] == '{}: transcript of 512 characters is too long to align (max 511)'.format(golden) and r['spans'] is None
  with pytest.raises(ValueError, match='confidences'):
    alignment.align_files(None, [golden], ['a'], segment=object(), confidence=True)


def test_concat_frame_seconds():
  from speecht_amd import alignment
  rate, pad = 16000, 0.1
  f2s = lambda f: alignment.frames_to_seconds(f, rate)          # 0.02 s per frame
  # three segments with 0.1 s of zeros on both sides (frames: (end - start + 0.2) / 0.02), the middle one too short for the features
  segments = [dict(start=0.05, end=1.05), dict(start=1.5, end=1.52), dict(start=2.0, end=3.0)]
  frames = [60, 0, 60]
  sec = lambda edges, **kw: alignment.concat_frame_seconds(edges, segments, frames, rate, pad, 3.05, **kw)
  assert sec([0]) == [0.0]                                       # 0.05 - 0.1: clipped to the file
  assert sec([10]) == [pytest.approx(0.05 - pad + f2s(10))]
  # frame 60 is the first frame of the third segment; as an end it is one past the last frame of the first
  assert sec([60]) == [pytest.approx(2.0 - pad)]
  assert sec([60], end=True) == [pytest.approx(0.05 - pad + f2s(60))]
  assert sec([120], end=True) == [3.05]                          # 2.0 - 0.1 + 1.2 = 3.1: clipped to the file
  with pytest.raises(ValueError):
    sec([120])
  with pytest.raises(ValueError):
    sec([0], end=True)
  starts, ends = sec(range(120)), sec(range(1, 121), end=True)
  both = [t for pair in zip(starts, ends) for t in pair]
  assert all(a <= b for a, b in zip(both, both[1:])) and 0.0 <= both[0] and both[-1] <= 3.05
  # two halves of an utterance cut at its quietest chunk: no gap for the pads, the times still do not run backwards
  segments = [dict(start=0.0, end=1.0), dict(start=1.0, end=2.0)]
  frames = [60, 60]
  starts, ends = sec(range(120)), sec(range(1, 121), end=True)
  both = [t for pair in zip(starts, ends) for t in pair]
  assert all(a <= b for a, b in zip(both, both[1:]))
  assert ends[59] == 1.0 and starts[60] == 1.0
  # timed_words on such an entry: a word that closes the first segment ends there, not at the start of the second
  ids = [0, 1]
  spans = np.array([[50, 60], [60, 70]], dtype=np.int32)
  segments = [dict(start=0.05, end=1.05), dict(start=2.0, end=3.0)]
  chars = alignment.timed_words(ids, spans, rate, 3.05, chars=True, concat=(segments, [60, 60], pad))
  assert chars[0]['end'] == pytest.approx(0.05 - pad + f2s(60)) and chars[1]['start'] == pytest.approx(1.9)
  assert alignment.concat_of(dict(spans=spans)) is None
