"""Silence segmentation without a GPU: the numpy specification (tests/segment_oracle.py) on hand-built signals with the answers
written out by hand, the stitching arithmetic of `segmentation.stitch`, and the command line's new flags.

Signals are built at rate 1000, so a chunk is 20 samples; a "loud" chunk is 20 samples of 1.0 (or the amplitude named), a silent
one 20 zeros.  The threshold 0.03 makes a sample active above 0.06 of the signal's peak."""
import importlib.machinery
import importlib.util
import os
import subprocess
import sys

import numpy as np

from tests import segment_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE, C = 1000, 20


def chunks(*amplitudes):
  return np.concatenate([np.full(C, a, np.float32) for a in amplitudes] + [np.zeros(0, np.float32)])


def seg(x, **kw):
  return O.segment_signal(x, RATE, **kw).tolist()


def test_parameters_in_chunks():
  assert O.chunk_size(1000) == 20 and O.chunk_size(16000) == 320 and O.chunk_size(22050) == 441 and O.chunk_size(30) == 1
  assert O.gap_chunks(0.3) == 15 and O.gap_chunks(0.1) == 5 and O.gap_chunks(0.0) == 1 and O.gap_chunks(0.05) == 3   # 2.5 rounds up
  assert O.max_chunks(20.0) == 1000 and O.max_chunks(0.2) == 10 and O.max_chunks(0.01) == 2


def test_gap_of_g_minus_one_joins_and_gap_of_g_splits():
  g = O.gap_chunks(0.1)                                     # 5
  joined = chunks(1, *([0] * (g - 1)), 1)
  assert seg(joined, min_silence=0.1) == [[0, (g + 1) * C]]
  split = chunks(1, *([0] * g), 1)
  assert seg(split, min_silence=0.1) == [[0, C], [(g + 1) * C, (g + 2) * C]]


def test_run_of_m_chunks_is_kept_and_m_plus_one_is_cut():
  m = O.max_chunks(0.2)                                     # 10
  assert seg(chunks(*([1] * m)), max_segment=0.2) == [[0, m * C]]
  # all chunks equal: the window is chunks [5, 10), the earliest of the equal minima is 5
  assert seg(chunks(*([1] * (m + 1))), max_segment=0.2) == [[0, 5 * C], [5 * C, 11 * C]]


def test_cut_lands_on_the_quietest_chunk_and_the_earliest_of_equals():
  amp = [1.0] * 11
  amp[7] = 0.5
  assert seg(chunks(*amp), max_segment=0.2) == [[0, 7 * C], [7 * C, 11 * C]]
  amp[8] = 0.5                                              # 7 and 8 tie: 7
  assert seg(chunks(*amp), max_segment=0.2) == [[0, 7 * C], [7 * C, 11 * C]]
  amp[6] = 0.5                                              # 6, 7 and 8 tie: 6
  assert seg(chunks(*amp), max_segment=0.2) == [[0, 6 * C], [6 * C, 11 * C]]
  amp[9] = 0.25                                             # quieter still, and the last chunk of the window
  assert seg(chunks(*amp), max_segment=0.2) == [[0, 9 * C], [9 * C, 11 * C]]
  # a silent chunk is the quietest: the left piece ends with the chunk before it, the rest starts with the next active one
  amp = [1.0] * 11
  amp[7] = 0.01
  assert seg(chunks(*amp), max_segment=0.2) == [[0, 7 * C], [8 * C, 11 * C]]


def test_repeated_cuts():
  # 25 equal chunks, M = 10: cut at 5 -> rest 20 chunks from 5: cut at 10 -> rest 15 from 10: cut at 15 -> rest 10 from 15, kept
  assert seg(chunks(*([1] * 25)), max_segment=0.2) == [[0, 100], [100, 200], [200, 300], [300, 500]]


def test_trim_is_sample_exact():
  x = np.zeros(100, np.float32)
  x[23], x[57], x[58] = 1.0, -0.5, 0.06                    # 0.06 is not above 2 * 0.03 * 1.0
  assert seg(x) == [[23, 58]]
  x[58] = np.nextafter(np.float32(0.06), np.float32(1))    # one float32 step above the threshold
  assert seg(x) == [[23, 59]]
  # the threshold follows the signal's peak
  assert seg(x * np.float32(0.25)) == [[23, 59]]


def test_all_zero_and_empty_signals_yield_nothing():
  assert seg(np.zeros(1000, np.float32)) == []
  assert seg(np.zeros(0, np.float32)) == []
  table, counts = O.segment([np.zeros(50, np.float32), chunks(1), np.zeros(0, np.float32)], [RATE] * 3)
  assert table.tolist() == [[1, 0, C]] and counts.tolist() == [0, 1, 0]


def test_gather_pads_and_normalises_to_half():
  x = np.zeros(100, np.float32)
  x[10:13] = [0.25, -0.8, 0.4]
  table, _ = O.segment([x], [RATE])
  assert table.tolist() == [[0, 10, 13]]
  (utt,), (rate,) = O.gather([x], [RATE], table)
  gain = np.float32(0.5) / np.float32(0.8)
  assert rate == RATE and utt.dtype == np.float32 and len(utt) == 100 + 3 + 100
  assert not utt[:100].any() and not utt[103:].any()
  assert utt[100:103].tolist() == [np.float32(0.25) * gain, np.float32(-0.8) * gain, np.float32(0.4) * gain]
  assert O.gather([x], [RATE], table, pad=0.0)[0][0].shape == (3,)


# ---- segmentation.stitch and the options -----------------------------------------------------------------------------------

def test_stitch_offsets_and_clipping():
  from speecht_amd.segmentation import stitch
  words = [dict(word='a', start=0.05, end=0.3), dict(word='b', start=0.3, end=0.62)]
  out = stitch(words, segment_start=10.0, pad_seconds=0.1, duration=10.4)
  assert out == [dict(word='a', start=9.95, end=10.2), dict(word='b', start=10.2, end=10.4)]        # 10.52 clipped to the file
  out = stitch(words, segment_start=0.02, pad_seconds=0.1, duration=5.0)
  assert out == [dict(word='a', start=0.0, end=0.22), dict(word='b', start=0.22, end=0.54)]         # -0.03 clipped to 0
  assert words[0] == dict(word='a', start=0.05, end=0.3)                                            # inputs untouched
  assert stitch([], 1.0, 0.1, 2.0) == []


def test_options_agree_with_the_specification():
  from speecht_amd import segmentation as S
  assert S.SegmentOptions() == (0.03, 0.3, 20.0, 0.1)
  for s in (0.0, 0.05, 0.1, 0.3, 0.31, 1.0, 2.5):
    assert S.gap_chunks(S.SegmentOptions(min_silence=s)) == O.gap_chunks(s)
  for s in (0.01, 0.2, 1.0, 20.0, 35.0):
    assert S.max_chunks(S.SegmentOptions(max_segment=s)) == O.max_chunks(s)
  assert [S.pad_samples(S.SegmentOptions(), r) for r in (1000, 8000, 16000, 22050, 44100)] == [100, 800, 1600, 2205, 4410]


def test_library_exports_the_segmentation_and_the_mask():
  from speecht_amd import _lib
  lib = _lib.load()
  for name in ('st_segment_chunks_f32', 'st_segment_runs', 'st_segment_gather_f32', 'st_mask_rows'):
    assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS, name


# ---- the command line ---------------------------------------------------------------------------------------------------

def _cli():
  loader = importlib.machinery.SourceFileLoader('speecht_cli_segment', os.path.join(ROOT, 'speecht-cli'))
  spec = importlib.util.spec_from_loader('speecht_cli_segment', loader)
  cli = importlib.util.module_from_spec(spec)
  loader.exec_module(cli)
  return cli


def test_cli_flags_default_to_off():
  cli = _cli()
  _, flags = cli.parse(['transcribe', 'x'])
  got = dict(vars(flags))
  added = dict(mask_padding=False, segment=False, segment_threshold=0.03, min_silence=0.3, max_segment=20.0)
  for key, value in added.items():
    assert got.pop(key) == value, key
  # what is left is the namespace of before
  assert got == dict(batch_size=1, beam_input=None, beam_width=0, command='transcribe', data_dir='data', device='cuda:0',
                     feature_type='power', language_model=None, lm_weight=0.8, log_dir='log', output=None, paths=['x'],
                     run_name='noname', run_train_dir='train/noname', run_type='other', sample_rate=22050, seed=None, timestamps=False,
                     train_dir='train', valid_word_count_weight=2.3, word_count_weight=0.0)
  _, flags = cli.parse(['align', 'x'])
  got = dict(vars(flags))
  assert got.pop('mask_padding') is False
  assert got == dict(batch_size=1, chars=False, command='align', data_dir='data', device='cuda:0', feature_type='power', log_dir='log',
                     output=None, paths=['x'], run_name='noname', run_train_dir='train/noname', run_type='other', sample_rate=22050,
                     seed=None, train_dir='train', transcripts=None)


def test_cli_flags_parse():
  cli = _cli()
  _, flags = cli.parse(['transcribe', '--segment', '--segment-threshold', '0.05', '--min-silence', '0.5', '--max-segment', '12',
                        '--mask-padding', '--batch-size', '16', 'a.wav'])
  assert (flags.segment, flags.segment_threshold, flags.min_silence, flags.max_segment, flags.mask_padding, flags.batch_size) == (
      True, 0.05, 0.5, 12.0, True, 16)
  _, flags = cli.parse(['align', '--mask-padding', '--batch-size', '4', 'a.wav'])
  assert flags.mask_padding and flags.batch_size == 4
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'speecht-cli'), 'transcribe', '--help'], capture_output=True, text=True,
                     timeout=120)
  assert r.returncode == 0 and '--segment --batch-size N --mask-padding' in ' '.join(r.stdout.split())
