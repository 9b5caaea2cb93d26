"""Float64 numpy statement of streaming recognition, written from the feature's description and not from the kernels: the
per-layer state machine on ``oracle.conv1d_same_fwd`` semantics, greedy decoding carried across steps, and the causal
normalisation of the mel features.  Checker only."""
import numpy as np

from oracle import w2l_oracle as O


def pad_left(width, stride):
  """Left part of SAME padding for T a multiple of the stride; tests assert it against ``O.same_padding`` for every T."""
  return O.same_padding(stride * 1000, width, stride)[1]


class LayerStream:
  """One layer, one stream.  Keeps only the input frames from ``e * stride - pad_left`` onwards (``base``: absolute index of
  the first kept frame); output j is emitted when j * stride - pad_left + width - 1 <= n - 1, or, after `finish`, for every
  j < ceil(n / stride) with frames outside [0, n) read as zero."""

  def __init__(self, filters, bias, stride, relu):
    self.F, self.b, self.stride, self.relu = np.asarray(filters, np.float64), np.asarray(bias, np.float64), stride, relu
    self.width, self.cin, self.cout = self.F.shape
    self.pl = pad_left(self.width, stride)
    self.n = self.e = self.base = 0
    self.kept = np.zeros((0, self.cin))
    self.max_kept = 0

  def _frame(self, t):
    if t < 0 or t >= self.n:
      return np.zeros(self.cin)
    assert t >= self.base, 'frame {} was dropped (base {})'.format(t, self.base)
    return self.kept[t - self.base]

  def push(self, frames, finished=False):
    frames = np.asarray(frames, np.float64).reshape(-1, self.cin)
    self.kept = np.concatenate([self.kept, frames])
    self.n += len(frames)
    out = []
    while True:
      j = self.e
      ready = j < -(-self.n // self.stride) if finished else j * self.stride - self.pl + self.width - 1 <= self.n - 1
      if not ready:
        break
      taps = np.stack([self._frame(j * self.stride - self.pl + w) for w in range(self.width)])     # [W, Cin]
      y = taps.reshape(-1) @ self.F.reshape(self.width * self.cin, self.cout) + self.b
      out.append(np.maximum(y, 0.0) if self.relu else y)
      self.e += 1
    new_base = max(self.e * self.stride - self.pl, 0)
    if new_base > self.base:
      self.kept = self.kept[new_base - self.base:]
      self.base = new_base
    self.max_kept = max(self.max_kept, len(self.kept))
    return np.stack(out) if out else np.zeros((0, self.cout))


class ModelStream:
  """The whole stack for one stream, with greedy decoding carried across steps."""

  def __init__(self, params, layers):
    self.layers = [LayerStream(F, b, s, relu) for (F, b), (W, s, cin, cout, relu) in zip(params, layers)]
    self.greedy = GreedyStream(layers[-1][3])
    self.total = 0
    self.first_row_at = None          # input frames received when the first logits row appeared

  def push(self, frames, finished=False):
    h = np.asarray(frames, np.float64)
    self.total += len(h)
    for l in self.layers:
      h = l.push(h, finished)
    if len(h) and self.first_row_at is None:
      self.first_row_at = self.total
    ids = self.greedy.push(h, self.total // 2 if finished else None)
    return h, ids


def run_stream(params, layers, x, chunks):
  """Feed x [T, C] in pieces of the given lengths, then finish -> (logits [T', C], ids, frames at the first row, model)."""
  m = ModelStream(params, layers)
  rows, ids, at = [], [], 0
  for c in chunks:
    h, i = m.push(x[at:at + c])
    at += c
    rows.append(h)
    ids += i
  assert at == len(x)
  h, i = m.push(x[:0], finished=True)
  rows.append(h)
  ids += i
  return np.concatenate(rows), ids, m.first_row_at, m


class GreedyStream:
  """tf.nn.ctc_greedy_decoder(merge_repeated=True) taken a few rows at a time: first maximum on ties, blank = C - 1, repeats
  merged and blanks dropped across calls; rows from ``limit`` on (known at the end) are not decoded."""

  def __init__(self, num_classes):
    self.C, self.prev, self.frames, self.score = num_classes, -1, 0, 0.0

  def push(self, rows, limit=None):
    ids = []
    for row in np.asarray(rows, np.float64).reshape(-1, self.C):
      if limit is not None and self.frames >= limit:
        break
      k = int(np.argmax(row))
      self.score -= row[k]
      if k != self.C - 1 and k != self.prev:
        ids.append(k)
      self.prev = k
      self.frames += 1
    return ids


def chunkings(T):
  """The feeds of the tests: single frames, sevens, ragged pieces with empty ones, all at once."""
  ragged = []
  left = T
  for c in (3, 0, 50, 1):
    c = min(c, left)
    ragged.append(c)
    left -= c
  ragged.append(left)
  return {'ones': [1] * T, 'sevens': [7] * (T // 7) + ([T % 7] if T % 7 else []), 'ragged': ragged, 'all': [T]}


def greedy_case():
  """Constructed logits [T, 5] (blank = 4) with a repeat, a blank and a tie straddling the boundaries of 1-, 2- and 3-row steps.
  Values are multiples of 1/4 so that every float sum of them is exact in any order."""
  ids = [1, 1, 4, 1, 2, 2, 2, 4, 4, 3, 0, 0, 3, 3, 4, 0, 1]
  x = np.full((len(ids), 5), -1.0)
  for t, k in enumerate(ids):
    x[t, k] = 0.25 * (t % 7 + 1)
  x[4, 3] = x[4, 2]          # tie between 2 and 3: the first maximum (2) wins, continuing the repeat into the next step
  x[9, 4] = x[9, 3]          # tie between 3 and the blank: 3 wins
  x[15, 0] = x[15, 2] = 1.5  # tie between 0 and 2: 0 wins
  expect = [1, 1, 2, 3, 0, 3, 0, 1]
  return x, expect


# ---- the mel front end ---------------------------------------------------------------------------------------------------

def _db(v, amin=1e-10):
  return 10.0 * np.log10(np.maximum(amin, v))


class FeatureStream:
  """Log-mel features of a stream of samples.  Frame t needs samples t * hop - 256 ... t * hop + 255, reflected at the start of
  the stream and, once it is finished, at its end.  Causal normalisation: with h(t) = max(t, warm - 1) (the last frame when the
  stream ends sooner), ref_t = the largest mel power over frames 0 ... h(t), x_t = max(dB(S_t) - dB(ref_t), -80), and mean_t /
  std_t the mean and population deviation of all x_t', t' <= h(t), each as it was computed; output (x_t - mean_t) / std_t.
  ``stats=(ref, mean, std)``: fixed statistics, no running update."""

  def __init__(self, samplerate, n_mels, warm=100, stats=None, n_fft=512, hop=160):
    self.basis = O.mel_filterbank(samplerate, n_fft, n_mels)
    self.window = O.hann_periodic(n_fft)
    self.n_fft, self.hop, self.warm, self.stats = n_fft, hop, warm, stats
    self.y = np.zeros(0)
    self.S = []                 # mel power of every frame so far
    self.x = []                 # x_t of every frame normalised so far
    self.done = 0               # frames put out

  def _sample(self, j, finished):
    n = len(self.y)
    if j < 0:
      j = -j
    if j >= n:
      assert finished, 'a frame was computed before its samples arrived'
      j = 2 * (n - 1) - j
    return self.y[j]

  def _frame(self, t, finished):
    half = self.n_fft // 2
    seg = np.array([self._sample(t * self.hop - half + k, finished) for k in range(self.n_fft)])
    spec = np.fft.rfft(seg * self.window)
    return self.basis @ (spec.real ** 2 + spec.imag ** 2)

  def push(self, samples, finished=False):
    self.y = np.concatenate([self.y, np.asarray(samples, np.float64)])
    n, half = len(self.y), self.n_fft // 2
    while True:
      t = len(self.S)
      ready = t < 1 + n // self.hop if finished else (t * self.hop + half - 1 <= n - 1 and half - t * self.hop <= n - 1)
      if not ready:
        break
      self.S.append(self._frame(t, finished))
    out = []
    if self.stats is not None:
      ref, mean, std = self.stats
      while self.done < len(self.S):
        x = np.maximum(_db(self.S[self.done]) - _db(ref), -80.0)
        out.append((x - mean) / std)
        self.done += 1
    else:
      while self.done < len(self.S):
        t = self.done
        h = max(t, self.warm - 1)
        if h >= len(self.S):
          if not finished:
            break
          h = len(self.S) - 1
        while len(self.x) <= h:                                  # x_u for u <= h: every one with the reference of ITS moment
          u = len(self.x)
          ref = np.max(np.stack(self.S[:max(u, min(self.warm - 1, h)) + 1]))
          self.x.append(np.maximum(_db(self.S[u]) - _db(ref), -80.0))
        seen = np.stack(self.x[:h + 1])
        out.append((self.x[t] - seen.mean()) / seen.std())
        self.done += 1
    return np.stack(out) if out else np.zeros((0, self.basis.shape[0]))


def stream_features(samplerate, n_mels, y, chunks, warm=100, stats=None):
  f = FeatureStream(samplerate, n_mels, warm, stats)
  at, rows = 0, []
  for c in chunks:
    rows.append(f.push(y[at:at + c]))
    at += c
  rows.append(f.push(y[at:], finished=True))
  return np.concatenate(rows)


def file_statistics(samplerate, n_mels, y):
  """(ref, mean, std) of the whole utterance: the constants ``calc_power_spectrogram`` normalises with."""
  S = O.mel_filterbank(samplerate, 512, n_mels) @ O.stft_power(y, 512, 160)
  db = O.power_to_db(S)
  return float(np.max(S)), float(db.mean()), float(db.std())
