"""Silence segmentation: cut recordings into utterances on the device (`speecht-cli transcribe --segment`).

The rules are the endpointing of the reference's `record` (record_utils.AudioRecorder: peak normalised to 0.5, samples with
abs(x) <= threshold trimmed from both ends, 0.1 s of zeros added on each side) applied to a whole recording: 20 ms chunks, a
silence of ``min_silence`` seconds ends an utterance, an utterance longer than ``max_segment`` seconds is cut at its quietest
chunk.  They are written out once in include/speecht_hip.h; tests/segment_oracle.py is their numpy specification, which the
kernels of csrc/segment.hip match bit for bit.  The audio goes to the device once; only the small segment tables come back,
and the gathered utterances stay there for the resampler and the features.
"""
import ctypes
from collections import namedtuple

import numpy as np

SegmentOptions = namedtuple('SegmentOptions', ['threshold', 'min_silence', 'max_segment', 'pad'])
SegmentOptions.__new__.__defaults__ = (0.03, 0.3, 20.0, 0.1)
SegmentOptions.__doc__ = """threshold: of the reference's `record` (a sample is active iff |x| > 2 * threshold * peak of its signal);
min_silence: seconds of silence that end an utterance; max_segment: longest utterance in seconds; pad: seconds of zeros added to
both ends of a gathered utterance."""

MAX_RATE = 1000000                      # (64 chunks of rate / 50 samples are indexed with an int)
_F32 = np.float32


def gap_chunks(options):
  """G of rule 3: round-half-up(min_silence * 50) chunks of 20 ms, at least 1 (float32 arithmetic, as the specification)."""
  return max(1, int(np.floor(_F32(options.min_silence) * _F32(50) + _F32(0.5))))


def max_chunks(options):
  """M of rule 4: floor(max_segment * 50) chunks, at least 2."""
  return max(2, int(np.floor(_F32(options.max_segment) * _F32(50))))


def pad_samples(options, rate):
  return int(_F32(options.pad) * _F32(rate))


def _check(options):
  if not (0 <= options.threshold < 0.5 and options.min_silence >= 0 and options.max_segment > 0 and options.pad >= 0):
    raise ValueError('SegmentOptions: threshold in [0, 0.5), min_silence >= 0, max_segment > 0, pad >= 0 expected, got {}'.format(
        options))
  if max_chunks(options) >= 2 ** 31 or gap_chunks(options) >= 2 ** 31:
    raise ValueError('SegmentOptions: {} is out of range'.format(options))


def segment_device(audio, offsets, rates, options=None):
  """Segment concatenated mono signals that are already on the device: ``audio`` a float32 device tensor, signal i at
  [offsets[i], offsets[i + 1]) (host int64 [n + 1]) with rate rates[i] (host) -- the layout of audio_io.resample_kaiser_best_device.

  Returns (table, gathered, out_offsets): ``table`` the host int64 [S, 3] rows (signal, start, end) in signal order and then
  time order (samples inside the signal); ``gathered`` a float32 device tensor with the S utterances -- peak 0.5, ``pad`` seconds
  of zeros on both sides -- one after the other, utterance s at [out_offsets[s], out_offsets[s + 1]) (host int64 [S + 1]), ready
  on the current stream for audio_io.resample_device and the feature functions.  The rate of utterance s is rates[table[s, 0]]."""
  import torch
  from . import _lib
  options = options or SegmentOptions()
  _check(options)
  dev = audio.device
  offsets = np.ascontiguousarray(offsets, dtype=np.int64)
  rates = np.ascontiguousarray(rates, dtype=np.int64)
  n = len(rates)
  if n == 0 or offsets.shape != (n + 1,) or offsets[0] != 0 or np.any(np.diff(offsets) < 0) or offsets[-1] > audio.numel():
    raise ValueError('segment_device: offsets must be n + 1 ascending sample offsets from 0 inside the audio buffer')
  if rates.min() <= 0 or rates.max() > MAX_RATE:
    raise ValueError('segment_device: rates must lie in 1..{}, got {}'.format(MAX_RATE, rates.tolist()))
  if audio.dtype != torch.float32 or not audio.is_contiguous() or audio.data_ptr() % 16:
    raise ValueError('segment_device: audio must be a contiguous, 16-byte aligned float32 device tensor')
  chunk = np.maximum(1, rates // 50)
  chunks = -(-np.diff(offsets) // chunk)
  group_offsets = np.zeros(n + 1, dtype=np.int64)
  group_offsets[1:] = np.cumsum(-(-chunks // 64))
  groups = int(group_offsets[-1])
  meta = torch.as_tensor(np.concatenate([offsets, group_offsets])).to(dev)
  d_rates = torch.as_tensor(rates.astype(np.int32)).to(dev)
  entries = max(64 * groups, 1)
  peaks = torch.empty(n, dtype=torch.float32, device=dev)
  chunk_peak = torch.empty(entries, dtype=torch.float32, device=dev)
  chunk_first = torch.empty(entries, dtype=torch.int32, device=dev)
  chunk_last = torch.empty(entries, dtype=torch.int32, device=dev)
  chunk_mask = torch.empty(max(groups, 1), dtype=torch.int64, device=dev)
  seg_ranges = torch.empty((entries, 2), dtype=torch.int64, device=dev)
  seg_peaks = torch.empty(entries, dtype=torch.float32, device=dev)
  seg_counts = torch.empty(n, dtype=torch.int32, device=dev)
  P = lambda t: ctypes.c_void_p(t.data_ptr())
  d_off, d_goff = ctypes.c_void_p(meta.data_ptr()), ctypes.c_void_p(meta.data_ptr() + 8 * (n + 1))
  stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
  threshold2 = float(_F32(2) * _F32(options.threshold))
  _lib.call('st_segment_chunks_f32', P(audio), d_off, P(d_rates), d_goff, n, groups, threshold2, P(peaks), P(chunk_peak),
            P(chunk_first), P(chunk_last), P(chunk_mask), stream)
  _lib.call('st_segment_runs', d_off, P(d_rates), d_goff, n, gap_chunks(options), max_chunks(options), P(chunk_peak), P(chunk_first),
            P(chunk_last), P(chunk_mask), P(seg_ranges), P(seg_peaks), P(seg_counts), stream)
  # the small tables come back: the counts, then the rows they say are there
  counts = seg_counts.cpu().numpy().astype(np.int64)
  total = int(counts.sum())
  table = np.zeros((total, 3), dtype=np.int64)
  out_offsets = np.zeros(total + 1, dtype=np.int64)
  if total == 0:
    return table, torch.empty(0, dtype=torch.float32, device=dev), out_offsets
  signal = np.repeat(np.arange(n, dtype=np.int64), counts)
  rows = 64 * group_offsets[signal] + (np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(counts) - counts, counts))
  d_rows = torch.as_tensor(rows).to(dev)
  table[:, 0] = signal
  table[:, 1:] = seg_ranges[d_rows].cpu().numpy()
  d_seg_peaks = seg_peaks[d_rows].contiguous()
  pads = np.array([pad_samples(options, r) for r in rates], dtype=np.int64)[signal]
  out_offsets[1:] = np.cumsum(table[:, 2] - table[:, 1] + 2 * pads)
  gmeta = torch.as_tensor(np.concatenate([offsets[signal] + table[:, 1], out_offsets])).to(dev)
  d_pads = torch.as_tensor(pads.astype(np.int32)).to(dev)
  n_out = int(out_offsets[-1])
  gathered = torch.empty(n_out, dtype=torch.float32, device=dev)
  _lib.call('st_segment_gather_f32', P(audio), ctypes.c_void_p(gmeta.data_ptr()), P(d_seg_peaks),
            ctypes.c_void_p(gmeta.data_ptr() + 8 * total), P(d_pads), total, n_out, P(gathered), stream)
  return table, gathered, out_offsets


def segment_audio(signals, rates, options=None, device='cuda:0'):
  """segment_device for host signals: float32 mono arrays at their own rates -> (table, gathered, out_offsets) as there."""
  import torch
  if len(signals) == 0 or len(signals) != len(rates):
    raise ValueError('segment_audio: one rate per signal expected ({} signals, {} rates)'.format(len(signals), len(rates)))
  offsets = np.concatenate([[0], np.cumsum([len(s) for s in signals])]).astype(np.int64)
  flat = np.concatenate([np.asarray(s, dtype=np.float32).reshape(-1) for s in signals] + [np.zeros(4, np.float32)])
  audio = torch.as_tensor(flat).to(torch.device(device))
  return segment_device(audio, offsets, rates, options)


def stitch(words, segment_start, pad_seconds, duration):
  """Word times inside a gathered segment -> times in the file: each of ``words`` ({word, start, end, ...} in seconds from the start
  of the padded segment) moves by the segment's start minus its leading pad and is clipped to [0, duration].  Pure arithmetic;
  returns new dicts."""
  shift = float(segment_start) - float(pad_seconds)
  clip = lambda t: round(min(max(float(t) + shift, 0.0), float(duration)), 4)
  return [dict(w, start=clip(w['start']), end=clip(w['end'])) for w in words]
