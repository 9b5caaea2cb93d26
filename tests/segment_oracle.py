"""Numpy specification of the silence segmentation (include/speecht_hip.h "Silence segmentation"; csrc/segment.hip).

Integer and float32 arithmetic only -- no float64 anywhere -- so that the device can match every table and every gathered sample
bit for bit.  Written for clarity, chunk by chunk; it is the checker, not a fast path.
"""
import numpy as np

F32 = np.float32


def gap_chunks(min_silence):
  """G: round-half-up(min_silence * 50) chunks, at least 1."""
  return max(1, int(np.floor(F32(min_silence) * F32(50) + F32(0.5))))


def max_chunks(max_segment):
  """M: floor(max_segment * 50) chunks, at least 2."""
  return max(2, int(np.floor(F32(max_segment) * F32(50))))


def chunk_size(rate):
  return max(1, int(rate) // 50)


def chunk_table(x, rate, threshold):
  """Rules 1-2 -> (peak of the signal, chunk peaks float32 [K], first / last active sample inside each chunk int64 [K], -1 where
  the chunk is silent)."""
  x = np.asarray(x, dtype=F32)
  n, c = len(x), chunk_size(rate)
  k = -(-n // c)
  mag = np.abs(x)
  peak = mag.max() if n else F32(0)
  thr = F32(F32(2) * F32(threshold)) * F32(peak)
  active = mag > thr
  peaks = np.zeros(k, F32)
  first = np.full(k, -1, np.int64)
  last = np.full(k, -1, np.int64)
  for j in range(k):
    lo, hi = j * c, min((j + 1) * c, n)
    peaks[j] = mag[lo:hi].max()
    where = np.flatnonzero(active[lo:hi])
    if len(where):
      first[j], last[j] = where[0], where[-1]
  return F32(peak), peaks, first, last


def runs(active, gap):
  """Rule 3 -> list of (first chunk, last chunk), both active and inclusive."""
  out, start, prev = [], None, None
  for j in np.flatnonzero(active):
    j = int(j)
    if start is None:
      start = j
    elif j - prev - 1 >= gap:
      out.append((start, prev))
      start = j
    prev = j
  if start is not None:
    out.append((start, prev))
  return out


def cut(run, active, peaks, most):
  """Rule 4 -> the pieces (first chunk, last ACTIVE chunk) of one run."""
  start, end = run
  pieces = []
  while end - start + 1 > most:
    lo, hi = start + most // 2, start + most
    j = lo + int(np.argmin(peaks[lo:hi]))          # (argmin: the first of equal minima)
    left = np.flatnonzero(active[start:j])
    pieces.append((start, start + int(left[-1])))
    start = j + int(np.flatnonzero(active[j:end + 1])[0])
  pieces.append((start, end))
  return pieces


def segment_signal(x, rate, threshold=0.03, min_silence=0.3, max_segment=20.0):
  """Rules 1-5 for one signal -> int64 [S, 2] sample ranges (start, end) in time order."""
  x = np.asarray(x, dtype=F32)
  if len(x) == 0:
    return np.zeros((0, 2), np.int64)
  peak, peaks, first, last = chunk_table(x, rate, threshold)
  if peak == 0:
    return np.zeros((0, 2), np.int64)
  c = chunk_size(rate)
  active = last >= 0
  rows = []
  for run in runs(active, gap_chunks(min_silence)):
    for a, b in cut(run, active, peaks, max_chunks(max_segment)):
      rows.append((a * c + int(first[a]), b * c + int(last[b]) + 1))
  return np.asarray(rows, dtype=np.int64).reshape(-1, 2)


def segment(signals, rates, threshold=0.03, min_silence=0.3, max_segment=20.0):
  """-> (int64 [S, 3] rows (signal, start, end) in signal order, then time order; int64 [n] segments per signal)."""
  rows, counts = [], []
  for i, (x, r) in enumerate(zip(signals, rates)):
    seg = segment_signal(x, r, threshold, min_silence, max_segment)
    counts.append(len(seg))
    rows += [(i, int(a), int(b)) for a, b in seg]
  return np.asarray(rows, dtype=np.int64).reshape(-1, 3), np.asarray(counts, dtype=np.int64)


def gather(signals, rates, table, pad=0.1):
  """Rule 6 -> (list of float32 utterances, their rates): pad zeros, x[start:end] * (float32(0.5) / segpeak), pad zeros."""
  out, out_rates = [], []
  for i, a, b in np.asarray(table, dtype=np.int64).reshape(-1, 3):
    x = np.asarray(signals[i], dtype=F32)[a:b]
    gain = F32(0.5) / np.abs(x).max()
    assert gain.dtype == F32
    z = np.zeros(int(F32(pad) * F32(rates[i])), F32)
    out.append(np.concatenate([z, x * gain, z]).astype(F32))
    out_rates.append(int(rates[i]))
  return out, out_rates
