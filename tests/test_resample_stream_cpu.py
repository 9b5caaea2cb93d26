"""Streamed kaiser_best resampling without a GPU: the readiness rule (audio_io.resample_ready / resample_need /
resample_stream_step), the host form st_resample_stream_host driven by `StreamingResampler(device='cpu')` against the offline host
form st_resample_kaiser_host, the status a table row gets when it breaks a bound, and the seconds <-> frames conversions called
without the new rate argument.

Every equality is exact: the streamed form runs the offline form's arithmetic (csrc/resample_map.h) in its order."""
import ctypes

import numpy as np
import pytest

from speecht_amd import _lib, audio_io
from speecht_amd.streaming import RS_ROW, Endpointing, StreamError, StreamingResampler, StreamSpotter

PAIRS = ((16000, 22050), (8000, 22050), (44100, 22050), (48000, 22050), (22050, 16000), (22050, 22050))
LENGTHS = (1, 2, 63, 64, 65, 129, 140, 279, 321, 5000)


def _p(a):
  return a.ctypes.data_as(ctypes.c_void_p)


def _limits(i, sr, new):
  """(n_i, wing 1's limit_i) for the outputs ``i``, computed as audio_io.resample_kaiser_best computes them."""
  ratio = float(new) / float(sr)
  scale = min(1.0, ratio)
  index_step = int(scale * 512)
  t = np.asarray(i, dtype=np.float64) / ratio
  n = t.astype(np.int64)
  frac = scale - scale * (t - n)
  offset = (frac * 512).astype(np.int64)
  return n, (32769 - offset) // index_step


_signals, _offline = {}, {}


def signal(n):
  if n not in _signals:
    _signals[n] = np.random.RandomState(n).uniform(-1, 1, n).astype(np.float32)
    _signals[n].setflags(write=False)
  return _signals[n]


def offline(n, sr, new):
  """st_resample_kaiser_host on the whole signal, float64 [target], computed once per case."""
  if (n, sr, new) not in _offline:
    y = signal(n)
    offs, valid = audio_io.plan_resample([n], [sr], new)
    ino, rates = np.array([0, n], np.int64), np.array([sr], np.int32)
    win = np.ascontiguousarray(audio_io._kaiser_best_filter()[0], dtype=np.float64)
    out = np.zeros(max(int(offs[-1]), 1))
    _lib.call('st_resample_kaiser_host', _p(y), _p(ino), 1, _p(rates), new, _p(offs), _p(valid), _p(win), len(win), _p(out))
    out = out[:offs[-1]]
    out.setflags(write=False)
    _offline[(n, sr, new)] = out
  return _offline[(n, sr, new)]


# ---- the rule ---------------------------------------------------------------------------------------------------------------

def test_taps():
  assert audio_io.resample_taps(16000, 22050) == 64 and audio_io.resample_taps(8000, 22050) == 64
  assert audio_io.resample_taps(48000, 22050) == 139 and audio_io.resample_taps(44100, 22050) == 128
  assert audio_io.resample_taps(22050, 22050) == 0
  with pytest.raises(ValueError):
    audio_io.resample_taps(22050 * 1024, 22050)


@pytest.mark.parametrize('sr,new', PAIRS)
def test_rule_at_every_count(sr, new):
  taps = audio_io.resample_taps(sr, new)
  ratio = float(new) / float(sr)
  last = 0
  for n in range(0, 3001):
    m = audio_io.resample_ready(n, sr, new)
    assert m >= last                                             # non-decreasing in N
    last = m
    if sr == new:
      assert m == n and audio_io.resample_need(m, sr, new) == m
      continue
    if m:
      n_i, limit = _limits(np.arange(m), sr, new)
      assert np.all(n_i + 1 + limit <= n) and np.all(limit <= taps)          # every final output has its whole right wing
    assert int(float(m) / ratio) + 1 + taps > n                  # the first one withheld breaks the rule
    assert audio_io.resample_need(m, sr, new) == max(int(float(m) / ratio) - taps, 0)
    assert n - audio_io.resample_need(m, sr, new) <= 2 * taps    # what a stream keeps between steps
    count, n_orig, valid, target = audio_io.resample_stream_step(n, m, 0, True, sr, new)
    assert (m + count, n_orig) == (audio_io.resample_lengths(n, sr, new)[1], n) == (target, n) and m <= valid <= target


def test_step_counts():
  assert audio_io.resample_stream_step(0, 0, 64, False, 16000, 22050) == (0, 0, 0, 0)
  assert audio_io.resample_stream_step(0, 0, 65, False, 16000, 22050) == (2, 0, 0, 0)      # outputs 0 and 1 sit on sample 0
  assert audio_io.resample_stream_step(100, 0, 60, False, 22050, 22050) == (160, 0, 0, 0)
  assert audio_io.resample_stream_step(0, 0, 3, True, 16000, 22050) == (5, 3, 4, 5)      # int(3 * 1.378125) = 4, ceil = 5


# ---- the host form against the offline host form ------------------------------------------------------------------------------

def chunkings(n):
  out = [[7] * (n // 7) + [n % 7], [160] * (n // 160) + [n % 160], [1601] * (n // 1601) + [n % 1601], [n], [0, n, 0]]
  if n <= 321:
    out.append([1] * n)
  return out


@pytest.mark.parametrize('sr,new', PAIRS)
def test_host_form_equals_offline(sr, new):
  taps = audio_io.resample_taps(sr, new)
  for n in LENGTHS:
    ref = offline(n, sr, new)
    y = signal(n)
    for chunks in chunkings(n):
      rs = StreamingResampler(new, 2, max_chunk_samples=1000, device='cpu')          # (1 601 and 5 000 are cut into passes)
      idle, s = rs.open(sr), rs.open(sr)
      got, got32, at = [], [], 0
      for c in chunks:
        got32.append(rs.step({s: y[at:at + c]})[s])
        got.append(rs.last64[s])
        at += c
        if sr != new and at <= taps:
          assert sum(len(g) for g in got) == 0                   # fewer than L + 1 samples: nothing is final yet
      assert at == n
      got32.append(rs.finish(s))
      got.append(rs.last64[s])
      got, got32 = np.concatenate(got), np.concatenate(got32)
      assert got.shape == ref.shape == (audio_io.resample_lengths(n, sr, new)[1],), (n, chunks[:3])
      assert np.array_equal(got, ref), (n, chunks[:3])
      assert got32.dtype == np.float32 and np.array_equal(got32, ref.astype(np.float32))
      with pytest.raises(StreamError, match='has been finished'):
        rs.step({s: y[:1]})
      rs.close(s)


def test_host_streams_together_and_reopened():
  """Streams of different rates in one call, ragged feeds, a slot reopened at another rate without clearing: each equals its own
  whole-signal result."""
  rs = StreamingResampler(22050, 4, max_chunk_samples=700, device='cpu')
  a, b, idle, c = rs.open(8000), rs.open(48000), rs.open(16000), rs.open(22050)
  ya, yb, yc = signal(321), signal(5000), signal(279)
  got = {a: [], b: [], c: []}
  for k in range(10):
    feeds = {b: yb[500 * k:500 * (k + 1)]}
    if k < 3:
      feeds[a] = ya[107 * k:107 * (k + 1)]
    if k % 2:
      feeds[c] = yc[56 * (k // 2):56 * (k // 2 + 1)]
    for s, out in rs.step(feeds).items():
      got[s].append(out)
    if k == 2:
      got[a].append(rs.finish(a))
      rs.close(a)
      assert rs.open(44100) == a                                 # the same slot, another rate, nothing cleared
      got['again'] = []
    if k > 2:
      got['again'].append(rs.step({a: signal(2100)[300 * (k - 3):300 * (k - 2)]})[a])
  got[b].append(rs.finish(b)), got[c].append(rs.finish(c)), got['again'].append(rs.finish(a))
  assert np.array_equal(np.concatenate(got[a]), offline(321, 8000, 22050).astype(np.float32))
  assert np.array_equal(np.concatenate(got[b]), offline(5000, 48000, 22050).astype(np.float32))
  assert np.array_equal(np.concatenate(got[c]), offline(279, 22050, 22050).astype(np.float32))
  assert np.array_equal(np.concatenate(got['again']), offline(2100, 44100, 22050).astype(np.float32))


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_requests_refused_before_anything_runs():
  rs = StreamingResampler(22050, 1, max_chunk_samples=100, device='cpu', max_source_rate=22050)
  with pytest.raises(StreamError, match='keeps 280 samples'):
    rs.open(48000)                                               # windows sized for up-sampling only
  with pytest.raises(StreamError, match='positive integer'):
    rs.open(0)
  s = rs.open(16000)
  with pytest.raises(StreamError, match='all 1 streams'):
    rs.open(16000)
  before = rs.state.copy()
  with pytest.raises(StreamError, match='a pass takes 100'):
    rs.step_device({s: np.zeros(101, np.float32)})
  with pytest.raises(StreamError, match='one-dimensional'):
    rs.step({s: np.zeros((2, 2), np.float32)})
  with pytest.raises(StreamError, match='not open'):
    rs.step({3: np.zeros(2, np.float32)})
  assert np.array_equal(rs.state, before) and (rs.slots[s].n, rs.slots[s].m) == (0, 0)
  assert len(rs.step({s: np.zeros(250, np.float32)})[s]) == audio_io.resample_ready(250, 16000, 22050)     # three passes


def _row(rate, base0, base1, n0, src, new, out0, count, off, fin=0, n_orig=0, valid=0, target=0, parity=0):
  r = np.zeros(RS_ROW, np.int64)
  r[:14] = (rate, base0, base1, n0, src, new, out0, count, off, fin, n_orig, valid, target, parity)
  return r


def test_status_rows():
  """A row that breaks a bound gets its status and writes nothing; the other rows of the call are served."""
  y = signal(321)
  ref = offline(321, 16000, 22050).astype(np.float32)
  m = audio_io.resample_ready(321, 16000, 22050)
  good = _row(16000, 0, audio_io.resample_need(m, 16000, 22050), 0, 0, 321, 0, m, 0)
  bad = {
      1: _row(16000, 0, 0, -1, 0, 321, 0, m, m),                                   # a negative counter
      2: _row(16000, 0, 0, 0, 0, 321, 0, m, m),                                    # would keep 321 samples in a window of 280
      3: _row(16000, 200, 257, 200, 0, 121, 0, m, m),                              # output 0 needs samples before position 0
      4: _row(16000, 0, audio_io.resample_need(m + 1, 16000, 22050), 0, 0, 321, 0, m + 1, m),     # one output too many
      5: _row(16000, 0, audio_io.resample_need(m, 16000, 22050), 0, 0, 321, 0, m, 2 * m),        # past the output buffer
      6: _row(22050 * 64, 0, 0, 0, 0, 10, 0, 0, m),                                # 4 096 taps a wing: no tile fits the LDS
  }
  for code, row in bad.items():
    rs = StreamingResampler(22050, 3, device='cpu')
    table = np.stack([good, row, np.zeros(RS_ROW, np.int64)])
    out, status = rs.run_table(table, y, 2 * m + 1, fill=7.0)
    assert status.tolist() == [0, code, 0], (code, status)
    assert np.array_equal(out[:m], ref[:m]) and np.all(out[m:] == 7.0), code
  rs = StreamingResampler(22050, 1, device='cpu')
  fin = _row(16000, 0, 321, 0, 0, 321, 0, len(ref), 0, 1, 321, 442, 443)
  out, status = rs.run_table(fin[None], y, len(ref))
  assert status.tolist() == [0] and np.array_equal(out, ref)
  for wrong in (_row(16000, 0, 321, 0, 0, 321, 0, len(ref), 0, 1, 320, 442, 443), _row(16000, 0, 321, 0, 0, 321, 0, len(ref), 0, 1, 321, 444, 443),
                _row(16000, 0, 321, 0, 0, 321, 0, len(ref) + 1, 0, 1, 321, 442, 443)):
    out, status = rs.run_table(wrong[None], y, len(ref) + 1, fill=7.0)
    assert status.tolist() == [4] and np.all(out == 7.0)


# ---- seconds <-> frames: the defaults are the parent's ---------------------------------------------------------------------------

def test_conversions_without_a_rate_are_unchanged():
  """Called without the rate argument the conversions return what they returned before it existed: ceil(seconds * 100 / stride -
  1e-9), at least 1 -- at the strides and seconds of the endpointing and spotting tests."""
  old = lambda seconds, stride: max(int(np.ceil(seconds * 100.0 / stride - 1e-9)), 1)
  for silence, lead, longest in ((0.5, 1.0, 30.0), (0.05, 0.1, 0.1), (0.001, 0.001, 0.001), (0.16, 0.4, 0.8), (0.1, 0.3, 1.5), (0.3, 2.0, 12.5)):
    for stride in (1, 2, 4):
      e = Endpointing(silence, lead, longest)
      want = (old(silence, stride), old(lead, stride), max(old(longest, stride), old(lead, stride)), 27)
      assert e.frames(stride, 29) == want == e.frames(stride, 29, None) == e.frames(stride, 29, 100.0)
  assert Endpointing().frames(2, 29) == (25, 50, 1500, 27) and Endpointing().frames(1, 29) == (50, 100, 3000, 27)
  assert Endpointing(0.05, 0.1, 0.1).frames(2, 29) == (3, 5, 5, 27)
  for hold in (0.3, 0.2, 0.05, 0.001, 1.0):
    for stride in (1, 2, 4):
      assert StreamSpotter(['a'], hold=hold).frames(stride) == old(hold, stride) == StreamSpotter(['a'], hold=hold).frames(stride, None)
  assert StreamSpotter(['a'], hold=0.3).frames(2) == 15
  # at the model's rate a frame lasts 160 / 22 050 s: 0.5 s of silence is 35 output frames of stride 2, not 25
  assert Endpointing().frames(2, 29, 22050 / 160.0) == (35, 69, 2068, 27)
  assert StreamSpotter(['a'], hold=0.3).frames(2, 22050 / 160.0) == 21


# ---- the command line -----------------------------------------------------------------------------------------------------------

def test_cli_model_rate_flag(capsys):
  import importlib.machinery
  import importlib.util
  import os
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  loader = importlib.machinery.SourceFileLoader('speecht_cli_resample_stream', os.path.join(root, 'speecht-cli'))
  spec = importlib.util.spec_from_loader('speecht_cli_resample_stream', loader)
  cli = importlib.util.module_from_spec(spec)
  loader.exec_module(cli)
  _, flags = cli.parse(['stream', 'a.flac'])
  assert flags.model_rate == 'native'                            # the default: nothing is resampled
  _, flags = cli.parse(['stream', '-', '--sample-rate', '8000', '--model-rate', '22050'])
  assert (flags.sample_rate, flags.model_rate) == (8000, 22050)
  for bad in ('0', 'fast'):
    with pytest.raises(SystemExit) as e:
      cli.main(['stream', 'a.flac', '--model-rate', bad])
    assert e.value.code == 2
  with pytest.raises(SystemExit):
    cli.main(['stream', '--help'])
  text = ' '.join(capsys.readouterr().out.split())
  assert '--model-rate' in text and '22050' in text and 'no resampling' in text and 'Greedy decoding, mel features, no resampling' not in text
