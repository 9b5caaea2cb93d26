"""Streaming recognition on the GPU (csrc/conv_stream.hip, speecht_amd/streaming.py): the product kernel alone on the model's
five layer shapes, the small model end to end at every length and chunking of the CPU test, ragged streams with a reopened
slot, the full-width model, greedy decoding across steps, the streaming mel front end, `speecht-cli stream`, and the requests
the session refuses.

Bounds: the product against ``O.conv1d_same_fwd`` of each stream alone within 2e-5 * max(1, max|y|) (the gate of
test_conv_fwd_bwd); logits within 1e-4 of the float64 oracle (the gate of test_small_train_step_vs_oracle_and_golden); between
chunkings, between a stream alone and among others, and between a row alone and among 65: bit for bit; features within 1e-3 of
tests/stream_oracle.py and of the whole-utterance kernel (the gate of test_melspec_vs_oracle)."""
import ctypes
import math

import numpy as np
import pytest

from oracle import w2l_oracle as O
from tests import stream_oracle as SO
from tests import workloads as WL

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 3, 47, 48, 97, 98, 99, 150, 151)
SMALL = WL.w2l_layers(16, width=24, fc=40)


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def make_engine(layers, dev):
  from speecht_amd.engine import Wav2LetterEngine
  return Wav2LetterEngine(layers, device=dev)


@pytest.fixture(scope='module')
def small(dev):
  params = WL.xavier_params(SMALL, seed=7)
  eng = make_engine(SMALL, dev)
  eng.set_weights(params)
  return eng, params


def stream_all(eng, x, chunks, max_chunk=64):
  from speecht_amd.streaming import transcribe_stream
  at, pieces = 0, []
  for c in chunks:
    pieces.append(x[at:at + c])
    at += c
  ids, partials, logits = transcribe_stream(eng, pieces, max_chunk_frames=max_chunk, return_logits=True)
  return ids, partials, logits


# ---- 1. the product kernel alone ---------------------------------------------------------------------------------------------

def _ptr(t):
  return ctypes.c_void_p(t.data_ptr())


class ConvCase:
  """Three streams of one layer with whole utterances in their windows: stream 0 (200 frames, its window starting at absolute
  frame 10), stream 1 (5 frames: fewer than the filter is wide where the filter has more than 5 taps), stream 2 (no row)."""

  def __init__(self, dev, W, s, cin, cout, relu):
    from speecht_amd import _lib
    self.lib = _lib
    rng = np.random.default_rng(W * 100 + cout)
    self.geo = (W, s, cin, cout, relu)
    F = rng.standard_normal((W, cin, cout)) * (1.0 / math.sqrt(W * cin))
    b = rng.standard_normal(cout) * 0.1
    self.eng = make_engine([(W, s, cin, cout, relu)], dev)
    self.eng.set_weights([(F, b)])
    self.spec = self.eng.layers[0]
    self.x = [rng.standard_normal((200, cin)), rng.standard_normal((5, cin)), rng.standard_normal((9, cin))]
    self.ref = [O.conv1d_same_fwd(x[None], F, b, s, relu)[0] for x in self.x]
    self.base = [10, 0, 0]
    self.cap = 200
    cp = self.spec.cin_pitch
    win = np.zeros((3, self.cap, cp), np.float32)
    win[:] = np.nan                                             # whatever lies outside [base, n) must never be read into a result
    for i, x in enumerate(self.x):
      win[i, :len(x) - self.base[i], :] = 0.0
      win[i, :len(x) - self.base[i], :cin] = x[self.base[i]:]
    self.win = torch.from_numpy(win).to(dev)
    self.info = torch.tensor([[self.base[i], len(self.x[i]), self.base[i], 0] for i in range(3)], dtype=torch.int32, device=dev)
    self.out_base = [len(self.ref[0]) - 70, 0, 0]               # the next layer's window of stream 0 starts 70 frames before the end
    self.out_info = torch.tensor([[self.out_base[i], 0, 0, 0] for i in range(3)], dtype=torch.int32, device=dev)
    self.out_cap = 100
    self.dev = dev

  def rows_for(self, n_rows):
    """The last outputs of stream 0 (they read the right padding) behind up to ceil(5 / stride) rows of stream 1."""
    W, s = self.geo[:2]
    t1 = -(-5 // s)
    r1 = min(t1, max(n_rows - 1, 0))
    t0 = len(self.ref[0])
    r0 = n_rows - r1
    return [(0, j) for j in range(t0 - r0, t0)] + [(1, j) for j in range(r1)]

  def run(self, rows, ws_bytes=None):
    W, s, cin, cout, relu = self.geo
    lib = self.lib.load()
    need = int(lib.st_stream_conv_ws(len(rows), W, self.spec.cin_pitch, cout))
    ws = torch.empty(max(need, 16) // 4, dtype=torch.float32, device=self.dev)
    pitch = self.spec.cout_pitch
    out = torch.full((3, self.out_cap, pitch), float('nan'), dtype=torch.float32, device=self.dev)
    table = torch.tensor(rows, dtype=torch.int32, device=self.dev).reshape(-1, 2)
    pf, pb = self.eng._slice(self.eng.params, 0)
    self.lib.call('st_stream_conv_f32', _ptr(self.win), self.cap, self.spec.cin_pitch, _ptr(self.info), _ptr(table), len(rows), 3,
                  _ptr(pf), _ptr(pb), W, s, cout, int(relu), _ptr(out), self.out_cap, pitch, _ptr(self.out_info), _ptr(ws),
                  need if ws_bytes is None else ws_bytes, self.eng.stream_ptr)
    torch.cuda.synchronize()
    return out.cpu().numpy()


LAYER_SHAPES = [(48, 2, 80, 250, True), (7, 1, 250, 250, True), (32, 1, 250, 2000, True), (1, 1, 2000, 2000, True),
                (1, 1, 2000, 29, False)]


@pytest.mark.parametrize('W,s,cin,cout,relu', LAYER_SHAPES)
def test_product_kernel_alone(dev, W, s, cin, cout, relu):
  case = ConvCase(dev, W, s, cin, cout, relu)
  outs = {}
  for n_rows in (1, 31, 32, 33, 65):
    rows = case.rows_for(n_rows)
    assert len(rows) == n_rows and all(j * s - (W - s) // 2 >= case.base[st] or st == 1 for st, j in rows)
    out = case.run(rows)
    outs[n_rows] = out
    written = np.zeros(out.shape[:2], bool)
    for st, j in rows:
      at = j - case.out_base[st]
      written[st, at] = True
      y, ref = out[st, at], case.ref[st][j]
      err = np.max(np.abs(y[:cout] - ref))
      assert err < 2e-5 * max(1.0, np.max(np.abs(case.ref[st]))), (n_rows, st, j, err)
      assert np.all(y[cout:] == 0), 'pad channels of a written row'
    assert np.all(np.isnan(out[~written])), 'a row outside the table was written'
    assert not written[2].any()
  # a row alone and among 65 (another row tile, another wave): bit for bit
  last = len(case.ref[0]) - 1 - case.out_base[0]
  np.testing.assert_array_equal(outs[1][0, last], outs[65][0, last])
  np.testing.assert_array_equal(outs[33][0, last], outs[65][0, last])
  np.testing.assert_array_equal(outs[33][1, 0], outs[65][1, 0])


def test_product_kernel_refuses_a_small_workspace(dev):
  from speecht_amd._lib import SpeechtHipError
  case = ConvCase(dev, 7, 1, 24, 24, True)
  rows = case.rows_for(33)
  with pytest.raises(SpeechtHipError, match='workspace too small'):
    case.run(rows, ws_bytes=1024)


# ---- 2. the small model end to end ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('T', LENGTHS)
def test_small_model_every_chunking(small, T):
  eng, params = small
  x = WL.synthetic_features(T, T, 16)
  ref = O.wav2letter_forward(x[None], params, SMALL)[:, 0]
  ref_ids, _ = O.ctc_greedy_decode(ref[:, None], [T // 2])
  gap = np.sort(ref[:T // 2], axis=1)
  safe = T // 2 == 0 or float(np.min(gap[:, -1] - gap[:, -2])) > 2e-4       # the oracle's decision is beyond the logits' bound
  got = {}
  for name, chunks in SO.chunkings(T).items():
    ids, partials, logits = stream_all(eng, x.astype(np.float32), chunks)
    assert logits.shape == ref.shape, name
    assert np.max(np.abs(logits - ref)) < 1e-4, (name, float(np.max(np.abs(logits - ref))))
    if safe:
      assert ids == ref_ids[0], name
    if name == 'ones' and T >= 99:                               # no row before 99 input frames, the first at 99
      assert partials[0][0] >= 99
    got[name] = (logits, ids)
  for name, (logits, ids) in got.items():
    assert np.array_equal(logits, got['all'][0]), name           # bit for bit between every pair of chunkings
    assert ids == got['all'][1], name


def test_first_row_arrives_at_99_frames(small):
  from speecht_amd.streaming import StreamingRecognizer
  eng, _ = small
  rec = StreamingRecognizer(eng, 1, max_chunk_frames=8)
  slot = rec.open()
  x = WL.synthetic_features(3, 120, 16).astype(np.float32)
  seen = []
  for t in range(120):
    r = rec.step({slot: x[t:t + 1]}, return_logits=True)
    seen.append(len(r.logits[slot]))
  assert sum(seen[:98]) == 0 and seen[98] == 1 and sum(seen) == 1 + (120 - 99) // 2
  assert rec.launches <= 11 * 2 + 3                              # products with their epilogues, feed, advance, decode


# ---- 3. ragged streams, a slot reopened ----------------------------------------------------------------------------------

def test_ragged_streams_equal_their_solo_runs(small):
  from speecht_amd.streaming import StreamingRecognizer
  eng, _ = small
  utt = {k: WL.synthetic_features(40 + i, n, 16).astype(np.float32) for i, (k, n) in enumerate((('a', 130), ('b', 60), ('c', 97), ('d', 75)))}
  solo = {k: stream_all(eng, x, [len(x)]) for k, x in utt.items()}
  rec = StreamingRecognizer(eng, 3, max_chunk_frames=32)
  slot = {k: rec.open() for k in 'abc'}
  got = {k: ([], []) for k in utt}
  at = dict.fromkeys(utt, 0)
  pace = {'a': 13, 'b': 30, 'c': 1, 'd': 25}

  def take(r, names):
    for k in names:
      got[k][0].extend(r.ids[slot[k]])
      got[k][1].append(r.logits[slot[k]])

  live, step = ['a', 'b', 'c'], 0
  while live:
    step += 1
    feeds = {}
    for k in live:
      n = 0 if (k == 'a' and step % 3 == 0) else pace[k]           # 'a' sometimes sends nothing
      feeds[slot[k]] = utt[k][at[k]:at[k] + n]
      at[k] += len(feeds[slot[k]])
    take(rec.step(feeds, return_logits=True), live)
    for k in list(live):
      if at[k] == len(utt[k]):
        take(rec.finish(slot[k], return_logits=True), [k])
        rec.close(slot[k])
        live.remove(k)
        if k == 'b':                                             # b's slot goes to a fourth utterance while the others run
          slot['d'] = rec.open()
          assert slot['d'] == slot['b']
          live.append('d')
  for k in utt:
    ids, _, logits = solo[k]
    assert np.array_equal(np.concatenate(got[k][1]), logits), k
    assert got[k][0] == ids, k


# ---- 4. full width -------------------------------------------------------------------------------------------------------

def test_full_width_two_streams(dev):
  from speecht_amd.streaming import StreamingRecognizer
  layers = WL.w2l_layers(80)
  params = WL.xavier_params(layers, seed=42)
  x, seq_lens, _ = WL.make_batch([201, 160], 80, seed=2)
  eng = make_engine(layers, dev)
  eng.set_weights(params)
  rec = StreamingRecognizer(eng, 2, max_chunk_frames=20)
  slots = [rec.open(), rec.open()]
  ids, rows = [[], []], [[], []]
  for at in range(0, 201, 20):
    feeds = {slots[i]: x[i, at:min(at + 20, seq_lens[i])].astype(np.float32) for i in range(2) if at < seq_lens[i]}
    r = rec.step(feeds, return_logits=True)
    for i in range(2):
      if slots[i] in feeds:
        ids[i] += r.ids[slots[i]]
        rows[i].append(r.logits[slots[i]])
  r = rec.finish_many(slots, return_logits=True)
  for i in range(2):
    ids[i] += r.ids[slots[i]]
    rows[i].append(r.logits[slots[i]])
    T = int(seq_lens[i])
    ref = O.wav2letter_forward(x[i:i + 1, :T], params, layers)[:, 0]           # the utterance ALONE
    logits = np.concatenate(rows[i])
    assert logits.shape == ref.shape
    assert np.max(np.abs(logits - ref)) < 1e-4
    # the oracle's top-two gap exceeds twice the logits' bound at every decoded frame for this seed (smallest: 8.0e-4 / 3.9e-4)
    top = np.sort(ref[:T // 2], axis=1)
    assert float(np.min(top[:, -1] - top[:, -2])) > 2e-4
    assert ids[i] == O.ctc_greedy_decode(ref[:, None], [T // 2])[0][0]


# ---- 5. greedy decoding across steps ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('step', (1, 2, 17))
def test_greedy_across_steps(dev, step):
  from speecht_amd import _lib
  from speecht_amd._lib import Tensor3
  x, expect = SO.greedy_case()
  T, C = x.shape
  padded = np.full((T, 32), 9.0, np.float32)                       # columns from C on hold larger values: they must not be looked at
  padded[:, :C] = x
  logits = torch.from_numpy(padded).to(dev)
  # the whole-utterance decoder on the concatenation
  desc = Tensor3(logits.data_ptr(), 1, T, C, 0, T, 32)
  lens = torch.tensor([T], dtype=torch.int32, device=dev)
  ref_ids = torch.zeros(T, dtype=torch.int32, device=dev)
  ref_len = torch.zeros(1, dtype=torch.int32, device=dev)
  ref_score = torch.zeros(1, dtype=torch.float32, device=dev)
  _lib.call('st_ctc_greedy_decode', ctypes.byref(desc), _ptr(lens), 1, _ptr(ref_ids), T, _ptr(ref_len), _ptr(ref_score), None)
  # ... and in steps, stream 1 of 3 (streams 0 and 2 sit idle)
  state = torch.full((3 * 4,), 77, dtype=torch.int32, device=dev)
  score = torch.full((3,), 5.0, dtype=torch.float64, device=dev)
  ids = torch.zeros(3 * T, dtype=torch.int32, device=dev)
  count = torch.zeros(3, dtype=torch.int32, device=dev)
  neg = torch.zeros(3, dtype=torch.float32, device=dev)
  got = []
  for at in range(0, T, step):
    n = min(step, T - at)
    rows = torch.tensor([[1, at + j] for j in range(n)], dtype=torch.int32, device=dev)
    table = torch.tensor([[0, 0, -1, 0], [0, n, -1, 1 if at == 0 else 0], [0, 0, -1, 0]], dtype=torch.int32, device=dev)
    _lib.call('st_ctc_greedy_stream', ctypes.c_void_p(logits.data_ptr() + at * 32 * 4), 32, C, _ptr(rows), _ptr(table), 3, _ptr(state),
              _ptr(score), _ptr(ids), T, _ptr(count), _ptr(neg), None)
    torch.cuda.synchronize()
    c = count.cpu().numpy()
    assert c[0] == 0 and c[2] == 0
    got += ids.view(3, T)[1, :c[1]].tolist()
  assert got == expect == ref_ids[:int(ref_len[0])].tolist()
  assert len(got) == int(ref_len[0])
  assert float(neg[1]) == float(ref_score[0])
  st = state.view(3, 4).cpu().numpy()
  assert st[1, 1] == T and st[1, 0] == int(np.argmax(x[-1])) and st[0, 0] == 77 and float(score[0]) == 5.0


# ---- 8. requests the session refuses ---------------------------------------------------------------------------------------

def test_bad_requests_leave_the_other_streams_alone(small):
  from speecht_amd.streaming import StreamError, StreamingRecognizer
  eng, _ = small
  x = WL.synthetic_features(77, 140, 16).astype(np.float32)
  ids_solo, _, logits_solo = stream_all(eng, x, [140])
  rec = StreamingRecognizer(eng, 2, max_chunk_frames=64)
  a, b = rec.open(), rec.open()
  rows, ids = [], []
  r = rec.step({a: x[:110]}, return_logits=True)
  rows.append(r.logits[a])
  ids += r.ids[a]
  with pytest.raises(StreamError, match='all 2 streams are open'):
    rec.open()
  rec.close(b)
  with pytest.raises(StreamError, match='not open'):
    rec.step({a: x[110:120], b: x[:5]})                          # a feed to a closed slot: nothing of the step runs, a's included
  with pytest.raises(StreamError, match=r'must be \[frames, 16\]'):
    rec.step({a: np.zeros((4, 17), np.float32)})
  with pytest.raises(StreamError, match='not open'):
    rec.finish(b)
  r = rec.step({a: x[110:]}, return_logits=True)
  rows.append(r.logits[a])
  ids += r.ids[a]
  r = rec.finish(a, return_logits=True)
  with pytest.raises(StreamError, match='has been finished'):
    rec.step({a: x[:3]})
  rows.append(r.logits[a])
  ids += r.ids[a]
  assert np.array_equal(np.concatenate(rows), logits_solo) and ids == ids_solo


# ---- 6. features -----------------------------------------------------------------------------------------------------------

def _golden_audio(golden_dir):
  import os
  from speecht_amd import audio_io
  y, sr = audio_io.librosa_load(os.path.join(golden_dir, '1089-134686-0037.flac'), sr=None)
  assert sr == 16000
  return np.asarray(y, np.float32)


def _stream_features(y, chunk, n_mels, dev, **kw):
  from speecht_amd.streaming import StreamingFeatures
  front = StreamingFeatures(16000, n_mels, max_streams=2, max_chunk_samples=4000, device=dev, **kw)
  idle, slot = front.open(), front.open()                        # slot 1 of 2: slot 0 stays open and idle
  rows = [front.step({slot: y[at:at + chunk]})[slot] for at in range(0, len(y), chunk)]
  rows.append(front.finish(slot))
  assert all(r.shape[1] == n_mels for r in rows)
  return np.concatenate(rows), [len(r) for r in rows]


@pytest.mark.parametrize('which', ('flac', 'synthetic'))
def test_features_running_statistics(dev, golden_dir, which):
  n_mels = 80
  y = _golden_audio(golden_dir) if which == 'flac' else O.synthetic_audio(12, 160 * 171 + 59).astype(np.float32)
  ref = SO.stream_features(16000, n_mels, y.astype(np.float64), [len(y)])
  got = {}
  for chunk in (1600, 3217, len(y)):
    got[chunk], counts = _stream_features(y, chunk, n_mels, dev)
    assert got[chunk].shape == ref.shape == (1 + len(y) // 160, n_mels)
    assert np.max(np.abs(got[chunk] - ref)) < 1e-3, (chunk, float(np.max(np.abs(got[chunk] - ref))))
    if chunk == 1600:                                            # nothing before frame 99 has arrived, then 100 frames at once
      first = next(i for i, c in enumerate(counts) if c)
      assert counts[first] >= 100 and (first + 1) * 1600 >= 99 * 160 + 256
  assert np.array_equal(got[1600], got[3217]) and np.array_equal(got[1600], got[len(y)])     # bit for bit between chunkings


def test_features_short_utterance_and_fixed_statistics(dev, golden_dir):
  from speecht_amd.preprocessing import calc_power_spectrogram
  n_mels = 80
  short = O.synthetic_audio(13, 160 * 80 + 7).astype(np.float32)                  # 81 frames <= warm
  offline = calc_power_spectrogram(short, 16000, n_mels=n_mels)
  for chunk in (1600, 3217, len(short)):
    got, _ = _stream_features(short, chunk, n_mels, dev)
    assert got.shape == offline.shape and np.max(np.abs(got - offline)) < 1e-3
  y = _golden_audio(golden_dir)
  offline = calc_power_spectrogram(y, 16000, n_mels=n_mels)
  stats = SO.file_statistics(16000, n_mels, y.astype(np.float64))
  a, counts = _stream_features(y, 1600, n_mels, dev, stats=stats)
  assert a.shape == offline.shape and np.max(np.abs(a - offline)) < 1e-3
  assert sum(counts[:3]) > 0                                     # fixed statistics: frames as soon as their samples are there
  b, _ = _stream_features(y, 3217, n_mels, dev, stats=stats)
  assert np.array_equal(a, b)


def test_features_refuse_bad_requests(dev):
  from speecht_amd.streaming import StreamError, StreamingFeatures
  front = StreamingFeatures(16000, 40, max_streams=1, max_chunk_samples=1000, device=dev)
  s = front.open()
  with pytest.raises(StreamError, match='all 1 streams are open'):
    front.open()
  with pytest.raises(StreamError, match='one-dimensional'):
    front.step({s: np.zeros((3, 2), np.float32)})
  front.step({s: np.zeros(200, np.float32)})
  with pytest.raises(StreamError, match='needs more than 256'):
    front.finish(s)
  with pytest.raises(StreamError, match='not open'):
    front.step({5: np.zeros(3, np.float32)})


# ---- 7. the command line -----------------------------------------------------------------------------------------------------

def test_cli_stream_end_to_end(dev, golden_dir, tmp_path, capsys, monkeypatch):
  import importlib.machinery
  import importlib.util
  import os
  from speecht_amd.speech_input import SingleInputLoader
  from speecht_amd.speech_model import Session, Wav2LetterModel
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  loader = importlib.machinery.SourceFileLoader('speecht_cli_stream_gpu', os.path.join(root, 'speecht-cli'))
  spec = importlib.util.spec_from_loader('speecht_cli_stream_gpu', loader)
  cli = importlib.util.module_from_spec(spec)
  loader.exec_module(cli)
  model = Wav2LetterModel(SingleInputLoader(128), 128, 29)       # a checkpoint written the way test_gpu_align.py does
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

  # the oracle first: does its greedy decision clear the logits' bound at every decoded frame of this file and seed?
  y = _golden_audio(golden_dir).astype(np.float64)
  feats = O.calc_power_spectrogram(y, 16000, n_mels=128)
  layers = WL.w2l_layers(128)
  ref = O.wav2letter_forward(feats[None], params, layers)[:, 0]
  top = np.sort(ref[:len(feats) // 2], axis=1)
  gap = float(np.min(top[:, -1] - top[:, -2]))
  assert gap > 2e-4, gap                                        # 5.3e-3 for this file and seed: twice the logits' bound is far away
  code, plain = run(['transcribe'] + base + ['--sample-rate', 'native', flac])
  assert code == 0 and len(plain) == 1
  code, lines = run(['stream'] + base + ['--normalize', 'file', flac])
  assert code == 0 and lines[-1].split('\t')[0] == flac
  for l in lines[:-1]:
    seconds, text = l.split('\t')
    assert 0.99 <= float(seconds) <= len(y) / 16000.0 + 1e-6 and lines[-1].split('\t', 1)[1].startswith(text)
  from speecht_amd import vocabulary
  assert lines[-1] == plain[0]
  assert lines[-1].split('\t', 1)[1] == vocabulary.ids_to_sentence(O.ctc_greedy_decode(ref[:, None], [len(feats) // 2])[0][0])
  code, lines = run(['stream'] + base + ['--chunk-ms', '330', flac])         # --normalize running
  assert code == 0 and lines[-1].startswith(flac + '\t')
  assert sorted(os.listdir(str(cwd))) == []                      # no train / data / log directory is created
