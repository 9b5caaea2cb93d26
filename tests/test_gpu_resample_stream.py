"""Streamed kaiser_best resampling on the GPU (csrc/resample_stream.hip, streaming.StreamingResampler): the kernel against the
offline kernel and the host form at every rate pair and chunking, tile and window edges, streams of different rates in one launch,
the requests and table rows it refuses, the mel front end fed at a source rate, and `speecht-cli stream --model-rate`.

Bounds: resampled samples bit for bit (the arithmetic and its order are the offline kernel's); features between chunkings bit for
bit, and against the whole-utterance feature kernel on the offline resampler's samples within 1e-3, the bound
test_gpu_stream.test_features_running_statistics uses for the same comparison at the native rate."""
import os

import numpy as np
import pytest

from oracle import w2l_oracle as O
from tests import workloads as WL

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

PAIRS = ((16000, 22050), (8000, 22050), (44100, 22050), (48000, 22050), (22050, 16000), (22050, 22050))


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


_signals, _offline, _host = {}, {}, {}


def signal(n):
  if n not in _signals:
    _signals[n] = np.random.RandomState(1000 + n).uniform(-1, 1, n).astype(np.float32)
    _signals[n].setflags(write=False)
  return _signals[n]


def offline(n, sr, new, dev):
  """The offline kernel's samples of the whole signal (st_resample_kaiser_f32), computed once per case."""
  from speecht_amd import audio_io
  if (n, sr, new) not in _offline:
    out = audio_io.resample_kaiser_best_batch([signal(n)], [sr], new, dev)[0].copy()
    out.setflags(write=False)
    _offline[(n, sr, new)] = out
  return _offline[(n, sr, new)]


def host_form(n, sr, new):
  """st_resample_stream_host's float32 samples, the signal fed in one piece and finished."""
  from speecht_amd.streaming import StreamingResampler
  if (n, sr, new) not in _host:
    rs = StreamingResampler(new, 1, max_chunk_samples=max(n, 1), device='cpu')
    s = rs.open(sr)
    _host[(n, sr, new)] = np.concatenate([rs.step({s: signal(n)})[s], rs.finish(s)])
  return _host[(n, sr, new)]


def streamed(rs, slot, y, chunk):
  parts = [rs.step({slot: y[at:at + chunk]})[slot] for at in range(0, len(y), chunk)]
  parts.append(rs.finish(slot))
  return np.concatenate(parts), [len(p) for p in parts]


# ---- 1. the kernel against the offline kernel and the host form ----------------------------------------------------------------

@pytest.mark.parametrize('sr,new', PAIRS)
def test_kernel_equals_offline_and_host(dev, sr, new):
  from speecht_amd.streaming import StreamingResampler
  rs = StreamingResampler(new, 2, max_chunk_samples=4000, device=dev)             # (5 000 in one piece is cut into two passes)
  idle = rs.open(16000)
  for n in (5000, 321):
    ref = offline(n, sr, new, dev)
    for chunk in (160, 1601, 3217, n):
      slot = rs.open(sr)
      got, counts = streamed(rs, slot, signal(n), chunk)
      rs.close(slot)
      assert got.dtype == np.float32 and got.shape == ref.shape, (n, chunk)
      assert np.array_equal(got, ref), (n, chunk, float(np.max(np.abs(got - ref))))
      assert np.array_equal(got, host_form(n, sr, new)), (n, chunk)
      if sr != new and chunk == 160:
        assert counts[0] > 0 and counts[-1] > 0                  # live: outputs as the samples come, a flush at the end


# ---- 2. tile and window edges -----------------------------------------------------------------------------------------------------

def _feed_for(rs, slot, want):
  """Samples to feed so that the slot's next step emits exactly ``want`` outputs (None: no feed size gives that count)."""
  from speecht_amd import audio_io
  st = rs.slots[slot]
  for new in range(1, 4 * want + 400):
    count = audio_io.resample_ready(st.n + new, st.rate, rs.model_rate) - st.m
    if count == want:
      return new
    if count > want:
      return None


@pytest.mark.parametrize('sr,new', ((16000, 22050), (48000, 22050)))
def test_tile_edges(dev, sr, new):
  """Steps of 255, 256, 257 and 513 outputs: one output short of a tile, a full tile, one past it, two tiles and one."""
  from speecht_amd.streaming import StreamingResampler
  y = signal(5000)
  ref = offline(5000, sr, new, dev)
  rs = StreamingResampler(new, 1, max_chunk_samples=4000, device=dev)
  slot = rs.open(sr)
  got, at, seen = [], 0, []
  for want in (255, 256, 257, 513):
    feed = _feed_for(rs, slot, want)
    while feed is None:                                          # up-sampling: a sample can add two outputs; move on by one
      got.append(rs.step({slot: y[at:at + 1]})[slot])
      at += 1
      feed = _feed_for(rs, slot, want)
    got.append(rs.step({slot: y[at:at + feed]})[slot])
    at += feed
    seen.append(len(got[-1]))
  assert seen == [255, 256, 257, 513] and at < len(y)
  got.append(rs.step({slot: y[at:]})[slot])
  got.append(rs.finish(slot))
  assert np.array_equal(np.concatenate(got), ref)


@pytest.mark.parametrize('sr,new', ((16000, 22050), (48000, 22050), (22050, 22050)))
def test_window_edges(dev, sr, new):
  from speecht_amd import audio_io
  from speecht_amd.streaming import StreamingResampler
  taps = audio_io.resample_taps(sr, new)
  rs = StreamingResampler(new, 1, max_chunk_samples=4000, device=dev)
  # the first step: wing 0 is cut by the signal's start; then a finish right after a step that emitted all it could
  slot = rs.open(sr)
  y, ref = signal(321), offline(321, sr, new, dev)
  first = rs.step({slot: y})[slot]
  assert len(first) == audio_io.resample_ready(321, sr, new) > 0 and np.array_equal(first, ref[:len(first)])
  assert len(rs.step({slot: y[:0]})[slot]) == 0                   # nothing new: nothing to emit
  rest = rs.finish(slot)
  assert np.array_equal(np.concatenate([first, rest]), ref)
  rs.close(slot)
  # fewer than L samples in all: everything comes at finish
  for n in (1, 10, 63):
    slot = rs.open(sr)
    y, ref = signal(n), offline(n, sr, new, dev)
    out = rs.step({slot: y})[slot]
    assert len(out) == (n if sr == new else 0) and n <= max(taps, 63)
    assert np.array_equal(np.concatenate([out, rs.finish(slot)]), ref)
    rs.close(slot)


# ---- 3. several streams in one launch -----------------------------------------------------------------------------------------------

def test_streams_of_four_rates_together(dev):
  """8, 16, 22.05 and 48 kHz streams in one launch, ragged feeds, one slot idle throughout, one closed and reopened at another rate
  without clearing: each stream equals its solo run and the offline kernel, bit for bit."""
  from speecht_amd.streaming import StreamingResampler
  rates = (8000, 16000, 22050, 48000)
  rs = StreamingResampler(22050, 5, max_chunk_samples=2000, device=dev)
  idle = rs.open(44100)
  slots = {r: rs.open(r) for r in rates}
  lengths = {8000: 500, 16000: 2500, 22050: 2500, 48000: 5000}
  steps = {8000: 173, 16000: 401, 22050: 700, 48000: 1000}
  got = {r: [] for r in rates}
  at = {r: 0 for r in rates}
  again, again_at = [], 0
  for k in range(10):
    feeds = {}
    for r in rates:
      if at[r] < lengths[r] and (k + r // 8000) % 3 != 0:        # ragged: every stream sits out every third step, at its own phase
        feeds[slots[r]] = signal(lengths[r])[at[r]:at[r] + steps[r]]
        at[r] += steps[r]
    if 8000 not in slots and again_at < 3100:                    # the reopened slot
      feeds[reopened] = signal(3100)[again_at:again_at + 517]
      again_at += 517
    out = rs.step(feeds)
    for r in rates:
      if r in slots and slots[r] in out:
        got[r].append(out[slots[r]])
    if 8000 not in slots and reopened in out:
      again.append(out[reopened])
    if 8000 in slots and at[8000] >= lengths[8000]:
      got[8000].append(rs.finish(slots[8000]))
      rs.close(slots.pop(8000))
      reopened = rs.open(16000)                                  # the slot the 8 kHz stream had; its windows are not cleared
  assert 8000 not in slots and again_at >= 3100
  for r in rates[1:]:
    assert at[r] >= lengths[r]
    got[r].append(rs.finish(slots[r]))
  again.append(rs.finish(reopened))
  assert rs.slots[idle].n == 0
  solo = StreamingResampler(22050, 1, max_chunk_samples=5000, device=dev)
  for r in rates:
    s = solo.open(r)
    alone = np.concatenate([solo.step({s: signal(lengths[r])})[s], solo.finish(s)])
    solo.close(s)
    assert np.array_equal(np.concatenate(got[r]), alone), r
    assert np.array_equal(alone, offline(lengths[r], r, 22050, dev)), r
  assert np.array_equal(np.concatenate(again), offline(3100, 16000, 22050, dev))


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals(dev):
  from speecht_amd import _lib, audio_io
  from speecht_amd.streaming import RS_ROW, StreamError, StreamingResampler
  rs = StreamingResampler(22050, 3, max_chunk_samples=1000, device=dev)
  s = rs.open(16000)
  with pytest.raises(StreamError, match='a pass takes 1000'):
    rs.step_device({s: np.zeros(1001, np.float32)})               # more than a pass holds: refused, nothing launched
  with pytest.raises(StreamError, match='not open'):
    rs.step({2: np.zeros(3, np.float32)})
  assert rs.launches == 0 and (rs.slots[s].n, rs.slots[s].m) == (0, 0)
  with pytest.raises(StreamError, match='does not fit the LDS'):
    StreamingResampler(22050, 1, device=dev, max_source_rate=22050 * 64).open(22050 * 64)

  def row(*fields):
    r = np.zeros(RS_ROW, np.int64)
    r[:len(fields)] = fields
    return r

  y = signal(321)
  ref = offline(321, 16000, 22050, dev)
  m = audio_io.resample_ready(321, 16000, 22050)
  need = audio_io.resample_need(m, 16000, 22050)
  good = row(16000, 0, need, 0, 0, 321, 0, m, 0)
  bad = {1: row(16000, 0, 0, -1, 0, 321, 0, m, m),                # a negative counter
         2: row(16000, 0, 0, 0, 0, 321, 0, m, m),                 # would keep 321 samples in a window of 280
         3: row(16000, 200, 257, 200, 0, 121, 0, m, m),           # output 0 needs samples before position 0
         4: row(16000, 0, audio_io.resample_need(m + 1, 16000, 22050), 0, 0, 321, 0, m + 1, m),   # one output too many
         5: row(16000, 0, need, 0, 0, 321, 0, m, 2 * m + 64)}     # past the output buffer
  for code, r in bad.items():
    out, status = rs.run_table(np.stack([good, r, np.zeros(RS_ROW, np.int64)]), y, 2 * m + 1, fill=7.0)
    assert status.tolist() == [0, code, 0], (code, status)
    assert np.array_equal(out[:m], ref[:m]) and np.all(out[m:] == 7.0), code        # the good row served, nothing else written
  launches = rs.launches
  with pytest.raises(_lib.SpeechtHipError, match='more than the LDS holds'):        # an error, and no launch
    rs.run_table(np.stack([good, row(22050 * 64, 0, 0, 0, 0, 10, 0, 0, m), np.zeros(RS_ROW, np.int64)]), y, m)
  assert rs.launches == launches


# ---- 5. the mel front end fed at a source rate ------------------------------------------------------------------------------------

def _golden(golden_dir):
  from speecht_amd import audio_io
  y, sr = audio_io.librosa_load(os.path.join(golden_dir, '1089-134686-0037.flac'), sr=None)
  assert sr == 16000
  return np.asarray(y, np.float32)


def _front(y, chunk, n_mels, dev, **kw):
  from speecht_amd.streaming import StreamingFeatures
  front = StreamingFeatures(22050, n_mels, max_streams=2, max_chunk_samples=4000, device=dev, source_rate=16000, **kw)
  idle, slot = front.open(), front.open()
  rows = [front.step({slot: y[at:at + chunk]})[slot] for at in range(0, len(y), chunk)]
  rows.append(front.finish(slot))
  return np.concatenate(rows), [len(r) for r in rows]


def test_front_end_at_a_source_rate(dev, golden_dir):
  """StreamingFeatures(22050, 80, source_rate=16000) on the golden FLAC: bit-identical between chunkings; with ``warm`` covering the
  file within 1e-3 of the whole-utterance features of the offline resampler's samples (device_features' two launches, at 80 mels --
  device_features itself is fixed at 128 mels and is compared at 128 below)."""
  from speecht_amd import audio_io, preprocessing, transcription
  y = _golden(golden_dir)
  frames = 1 + audio_io.resample_lengths(len(y), 16000, 22050)[1] // 160
  got = {}
  for chunk in (1600, 3217, len(y)):
    got[chunk], counts = _front(y, chunk, 80, dev)
    assert got[chunk].shape == (frames, 80)
    if chunk == 1600:
      assert sum(1 for c in counts if c) > 3                      # live: features keep coming as the samples do
  assert np.array_equal(got[1600], got[3217]) and np.array_equal(got[1600], got[len(y)])
  whole = {c: _front(y, c, 80, dev, warm=frames)[0] for c in (1600, 3217, len(y))}
  assert np.array_equal(whole[1600], whole[3217]) and np.array_equal(whole[1600], whole[len(y)])
  audio, offsets = audio_io.resample_kaiser_best_device([y], [16000], 22050, dev)
  ref = preprocessing.power_spectrogram_device(audio, offsets, 22050, n_mels=80)[0]
  err = float(np.max(np.abs(whole[1600] - ref)))
  print('front end, 80 mels, against the whole-utterance kernel:', err)
  assert whole[1600].shape == ref.shape and err < 1e-3, err
  ref = transcription.device_features([y], [16000], 'power', 22050, device=dev)[0]
  wide = _front(y, 3217, 128, dev, warm=frames)[0]
  err = float(np.max(np.abs(wide - ref)))
  print('front end, 128 mels, against device_features:', err)
  assert wide.shape == ref.shape and err < 1e-3, err


def test_front_end_without_a_source_rate_is_unchanged(dev, golden_dir):
  """No source rate: no resampler is built, and the features equal those of a front end whose streams pass through the resampler
  at equal rates (a copy), bit for bit."""
  from speecht_amd.streaming import StreamingFeatures
  y = _golden(golden_dir)[:16000]
  plain = StreamingFeatures(16000, 40, max_streams=1, max_chunk_samples=4000, device=dev)
  s = plain.open()
  a = np.concatenate([plain.step({s: y})[s], plain.finish(s)])
  assert plain.resampler is None
  copy = StreamingFeatures(16000, 40, max_streams=1, max_chunk_samples=4000, device=dev, source_rate=16000)
  s = copy.open()
  b = np.concatenate([copy.step({s: y})[s], copy.finish(s)])
  assert copy.resampler is not None and np.array_equal(a, b)


# ---- 6. the command line ----------------------------------------------------------------------------------------------------------

def test_cli_stream_model_rate(dev, golden_dir, tmp_path, capsys, monkeypatch):
  import importlib.machinery
  import importlib.util
  from speecht_amd import audio_io, vocabulary
  from speecht_amd.speech_input import SingleInputLoader
  from speecht_amd.speech_model import Session, Wav2LetterModel
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  loader = importlib.machinery.SourceFileLoader('speecht_cli_resample_stream_gpu', os.path.join(root, 'speecht-cli'))
  spec = importlib.util.spec_from_loader('speecht_cli_resample_stream_gpu', loader)
  cli = importlib.util.module_from_spec(spec)
  loader.exec_module(cli)
  model = Wav2LetterModel(SingleInputLoader(128), 128, 29)       # the checkpoint of test_gpu_stream.test_cli_stream_end_to_end
  model.add_training_ops()
  model.add_decoding_ops()
  model.finalize(str(tmp_path / 'log'), 'r', 'record')
  model.init_seed = 1234
  train = tmp_path / 'train'
  (train / 'run').mkdir(parents=True)
  with Session(dev) as sess:
    model.init_session(sess)
    model.saver.save(sess, str(train / 'run' / 'speechT'), global_step=model.global_step)
    params = [(np.asarray(F, np.float64), np.asarray(b, np.float64)) for F, b in model.engine.get_weights()]
  flac = os.path.join(golden_dir, '1089-134686-0037.flac')
  cwd = tmp_path / 'cwd'
  cwd.mkdir()
  monkeypatch.chdir(cwd)
  base = ['--train-dir', str(train), '--run-name', 'run', '--device', dev]

  def run(args):
    capsys.readouterr()
    code = cli.main(args)
    return code, capsys.readouterr().out.splitlines()

  # the oracle first, at the model's rate: does its greedy decision clear the logits' bound at every decoded frame?
  y22, rate = audio_io.librosa_load(flac, sr=22050)
  assert rate == 22050
  duration = len(_golden(golden_dir)) / 16000.0
  feats = O.calc_power_spectrogram(y22.astype(np.float64), 22050, n_mels=128)
  ref = O.wav2letter_forward(feats[None], params, WL.w2l_layers(128))[:, 0]
  top = np.sort(ref[:len(feats) // 2], axis=1)
  gap = float(np.min(top[:, -1] - top[:, -2]))
  print('greedy gap of the oracle at 22 050 Hz:', gap)
  assert gap > 2e-4, gap                                        # twice the logits' bound, as test_cli_stream_end_to_end asks
  code, plain = run(['transcribe'] + base + [flac])              # 22 050 Hz and batch size 1 by default
  assert code == 0 and len(plain) == 1
  code, lines = run(['stream'] + base + ['--normalize', 'file', '--model-rate', '22050', flac])
  assert code == 0 and lines[-1] == plain[0]
  assert lines[-1].split('\t', 1)[1] == vocabulary.ids_to_sentence(O.ctc_greedy_decode(ref[:, None], [len(feats) // 2])[0][0])
  for l in lines[:-1]:
    seconds, text = l.split('\t')
    assert 0.0 < float(seconds) <= duration + 1e-3 and lines[-1].split('\t', 1)[1].startswith(text)
  # utterance times count frames of 160 / 22 050 s: none lies past the end of the file (with 10 ms frames they would, by 1.38 x)
  code, lines = run(['stream'] + base + ['--model-rate', '22050', '--endpoint', '--endpoint-silence', '0.1', '--endpoint-lead', '0.3',
                                         '--max-utterance', '1.5', flac])
  utts = [l.split('\t') for l in lines if l.startswith('utt\t')]
  assert code == 0 and utts and lines[-1].startswith(flac + '\t')
  for u in utts:
    assert 0.0 <= float(u[2]) <= float(u[3]) <= duration + 1e-6, (u, duration)
  # without the flag nothing changes: the default is native
  code, default = run(['stream'] + base + ['--chunk-ms', '330', flac])
  code2, native = run(['stream'] + base + ['--chunk-ms', '330', '--model-rate', 'native', flac])
  assert code == 0 and code2 == 0 and default == native and default[-1].startswith(flac + '\t')
  assert sorted(os.listdir(str(cwd))) == []
