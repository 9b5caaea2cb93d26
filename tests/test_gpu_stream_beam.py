"""The CTC beam searches carried across steps (st_ctc_beam_stream_step / _read, StreamingRecognizer(beam=...), `speecht-cli stream
--language-model`): however a stream's rows are cut, the finishing read returns the ids, the length and -- bit for bit -- the
log-probability of the whole-utterance searches on the same rows; partial hypotheses and stable lengths equal the float64
specification (tests/stream_beam_oracle.py) on inputs tests/test_stream_beam_cpu.py has vetted; slots are reused; the node pool is
never overrun; the layers above; the requests the entry points refuse."""
import ctypes
import os

import numpy as np
import pytest

from tests import stream_beam_cases as SC
from tests import workloads as WL
from tests.test_gpu_lm_beam import TINY, _engine, _model

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A5A5A5A5A
CUTS = (1, 2, 7, 10, 80)
WEIGHTS = (0.8, 0.0, 2.3, -1000.0)


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def _ptr(t):
  return ctypes.c_void_p(t.data_ptr())


def _f(values):
  return [ctypes.c_float(v) for v in values]


class Harness:
  """B streams through the C ABI with the host's part of the contract: the labels below a stream's stable length are kept from
  earlier reads, a read appends the reported tail.  State and pool start as garbage (the first step resets); the pool lies inside
  a larger tensor whose tail holds a pattern; the logits' columns from C on hold values the kernels must not look at."""

  def __init__(self, dev, logits, lens, beam, lm=None, transform=0, max_frames=80, max_tail=96):
    from speecht_amd import _lib
    self.lib, self.raw = _lib, _lib.load()
    self.dev, self.logits, self.lens = dev, logits, [int(n) for n in lens]
    self.T, self.S, self.C = logits.shape
    self.beam, self.lm, self.transform, self.max_frames, self.max_tail = beam, lm, transform, max_frames, max_tail
    self.handle = lm.device_handle(dev) if lm is not None else None
    self.state_bytes = int(self.raw.st_ctc_beam_stream_state_bytes(beam, int(lm is not None)))
    self.pool_bytes = int(self.raw.st_ctc_beam_stream_pool_bytes(max_frames, beam))
    assert self.state_bytes % 8 == 0 and self.pool_bytes % 8 == 0 and self.pool_bytes >= 8 * (max_frames * beam + 1)
    self.state = torch.full((self.S * self.state_bytes // 8,), PATTERN, dtype=torch.int64, device=dev)
    self.pool = torch.full((self.S * self.pool_bytes // 8 + 64,), PATTERN, dtype=torch.int64, device=dev)
    self.ws_rows = self.S * (self.T + 4)
    self.ws_bytes = int(self.raw.st_ctc_beam_stream_ws(self.ws_rows))
    self.ws = torch.empty(self.ws_bytes // 4, dtype=torch.float32, device=dev)
    self.tail = torch.zeros(self.S * max_tail, dtype=torch.int32, device=dev)
    self.result = torch.zeros(self.S * 4, dtype=torch.int32, device=dev)
    self.fed, self.started = [0] * self.S, [False] * self.S
    self.hyp, self.stable, self.logp, self.status = [[] for _ in range(self.S)], [0] * self.S, [None] * self.S, [0] * self.S

  def step(self, takes, finishing=(), read=True, extra=0):
    """``takes``: {stream: rows}; a finishing stream gets its limit and ``extra`` rows past it (which must not be decoded)."""
    rows, table, chunks = [], np.zeros((self.S, 4), np.int32), []
    table[:, 2] = -1
    for s in sorted(set(takes) | set(finishing)):
      n = takes.get(s, 0)
      if s in finishing:
        n += min(extra, self.T - self.fed[s] - n)
      table[s] = (len(rows), n, self.lens[s] if s in finishing else -1, 0 if self.started[s] else 1)
      rows += [(s, self.fed[s] + j) for j in range(n)]
      chunks.append(self.logits[self.fed[s]:self.fed[s] + n, s])
      self.fed[s] += n
      self.started[s] = True
    n_rows = len(rows)
    buf = np.full((max(n_rows, 1), 32), 9.0, np.float32)
    if n_rows:
      buf[:n_rows, :self.C] = np.concatenate(chunks)
    d_buf = torch.from_numpy(buf).to(self.dev)
    d_rows = torch.tensor(rows if rows else [(0, 0)], dtype=torch.int32, device=self.dev)
    d_table = torch.from_numpy(table).to(self.dev)
    self.lib.call('st_ctc_beam_stream_step', _ptr(d_buf), 32, self.C, _ptr(d_rows), _ptr(d_table), n_rows, self.S, self.beam, self.transform,
                  self.handle, *_f(WEIGHTS), _ptr(self.state), _ptr(self.pool), self.max_frames, _ptr(self.ws), self.ws_bytes, None)
    if read:
      self.read(d_table)
    return d_table

  def read(self, d_table):
    self.lib.call('st_ctc_beam_stream_read', _ptr(d_table), self.S, self.beam, self.handle, *_f(WEIGHTS), _ptr(self.state), _ptr(self.pool),
                  self.max_frames, _ptr(self.tail), self.max_tail, _ptr(self.result), None)
    torch.cuda.synchronize()
    table = d_table.cpu().numpy()
    res, tail = self.result.cpu().numpy().reshape(self.S, 4), self.tail.cpu().numpy().reshape(self.S, self.max_tail)
    for s in range(self.S):
      if table[s, 1] > 0 or table[s, 2] >= 0 or table[s, 3]:
        length, old = int(res[s, 0]), self.stable[s]
        assert 0 <= length - old <= self.max_tail, (s, length, old)
        self.hyp[s] = self.hyp[s][:old] + tail[s, :length - old].tolist()
        self.stable[s], self.logp[s], self.status[s] = int(res[s, 1]), res[s, 2:3].view(np.float32)[0], int(res[s, 3])
        assert self.stable[s] >= old

  def run(self, cuts, read_every_step=True, on_step=None):
    """Stream s takes cuts[s] rows per step until its length is fed; the step that feeds its last rows finishes it."""
    live, k = set(range(self.S)), 0
    while live:
      takes, finishing = {}, set()
      for s in sorted(live):
        n = min(cuts[s], self.lens[s] - self.fed[s])
        takes[s] = n
        if self.fed[s] + n >= self.lens[s]:
          finishing.add(s)
      table = self.step(takes, finishing, read=read_every_step or bool(finishing), extra=3)
      if on_step:
        on_step(k, takes, finishing)
      live -= finishing
      k += 1
    return [list(h) for h in self.hyp], np.asarray(self.logp, np.float32)

  def pattern_intact(self):
    return bool((self.pool[self.S * self.pool_bytes // 8:] == PATTERN).all())


def _offline(dev, logits, lens, beam, lm, transform):
  eng = _engine(dev, logits, lens)
  name = 'log10_softmax' if transform else None
  if lm is None:
    return eng.beam_search_decode(beam, name)
  return eng.lm_beam_search_decode(lm, beam, name, *WEIGHTS)


def _inputs(kind, beam):
  if kind == 'free5':
    return SC.cases5(beam)
  return SC.cases29(10 * beam + (int(kind) if kind != 'free' else 0))


# ---- 1. the kernels through the C ABI ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('transform', [0, 1])
@pytest.mark.parametrize('kind', ['free', 'free5', '1', '3', '5'])
@pytest.mark.parametrize('beam', [1, 16, 64, 100, 128])
def test_every_cut_returns_the_whole_utterance_search_bit_for_bit(dev, tmp_path_factory, beam, kind, transform):
  from speecht_amd._lib import launch_trace
  logits, lens = _inputs(kind, beam)
  lm = _model(str(tmp_path_factory.getbasetemp()), int(kind))[0] if kind.isdigit() else None
  ref_ids, ref_lp = _offline(dev, logits, lens, beam, lm, transform)
  for shift in (0, 2):                                            # the streams run side by side, each with another cut
    cuts = [CUTS[(s + shift) % len(CUTS)] for s in range(len(lens))]
    h = Harness(dev, logits, lens, beam, lm, transform)
    with launch_trace() as tr:
      ids, lp = h.run(cuts)
    want = 'ctc_beam_stream_lm<' if lm is not None else 'ctc_beam_stream<'
    assert any(l.startswith(want + ('wide' if beam > 64 else 'wave')) for l in tr.lines), tr.lines[:4]
    assert any(l.startswith('ctc_beam_stream_read<') for l in tr.lines)
    assert ids == ref_ids, (cuts, ids, ref_ids)
    assert lp.tobytes() == np.asarray(ref_lp, np.float32).reshape(-1).tobytes(), (cuts, lp, ref_lp)
    assert h.status == [0] * len(lens) and h.pattern_intact()
  assert ids[3] == []


# ---- 2. partial results ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', [c[0] for c in SC.EXACT])
def test_partials_equal_the_specification(dev, name):
  logits, lens, beam, order, transform = SC.exact_inputs(name)
  lm = _model(None, order)[0] if order else None
  spec = SC.traces(name)
  code = 1 if transform else 0
  h = Harness(dev, logits, lens, beam, lm, code)
  checked = [0]

  def check(k, takes, finishing):
    for s in takes:
      if s in finishing:
        continue                                                  # (the finishing read reports the whole-utterance result)
      n = h.fed[s]
      assert h.hyp[s] == spec[s]['hyp'][n], (name, s, n)
      assert h.stable[s] == spec[s]['stable'][n], (name, s, n)
      checked[0] += 1

  ids, lp = h.run([7, 2, 10, 1, 1], on_step=check)
  assert checked[0] > 20
  assert ids == [tr['final'][0] for tr in spec]
  np.testing.assert_allclose(lp, [tr['final'][1] for tr in spec], rtol=1e-4, atol=1e-4)   # the bound the offline searches' tests hold log_prob to
  # a read-out changes nothing for the later steps: a run that reads only when a stream finishes returns the same bits
  quiet = Harness(dev, logits, lens, beam, lm, code)
  ids2, lp2 = quiet.run([7, 2, 10, 1, 1], read_every_step=False)
  assert ids2 == ids and lp2.tobytes() == lp.tobytes()


# ---- 4b. the pool's capacity through the C ABI -----------------------------------------------------------------------------

@pytest.mark.parametrize('beam,kind', [(16, 'free'), (100, '3')])
def test_rows_past_the_pool_are_refused_not_written(dev, beam, kind):
  logits, lens = _inputs(kind, beam)
  lm = _model(None, 3)[0] if kind == '3' else None
  lens = [80, 12, 16, 0, 1]                                       # stream 2 fills its pool exactly
  small = Harness(dev, logits, lens, beam, lm, 0, max_frames=16)
  small.step({0: 10, 1: 12, 2: 16, 4: 1}, finishing={1, 2, 3, 4})
  assert small.status == [0] * 5
  small.step({0: 10})                                             # frames 10..19 of stream 0: 16..19 are past the pool
  assert small.status[0] & 1 and small.pattern_intact()
  small.step({0: 5})                                              # ... and so is everything after them
  assert small.status[0] & 1 and small.pattern_intact()
  big = Harness(dev, logits, lens, beam, lm, 0, max_frames=80)
  big.step({0: 10, 1: 12, 2: 16, 4: 1}, finishing={1, 2, 3, 4})
  big.step({0: 6})
  for s in range(5):                                              # the frames within capacity are decoded as before
    assert small.hyp[s] == big.hyp[s] and small.stable[s] == big.stable[s], s
    assert np.float32(small.logp[s]).tobytes() == np.float32(big.logp[s]).tobytes(), s


# ---- 6. the requests the entry points refuse -------------------------------------------------------------------------------

def test_validation_returns_an_error_without_a_launch(dev):
  from speecht_amd import _lib
  from speecht_amd._lib import launch_trace
  from speecht_amd.language_model import LanguageModel
  lib = _lib.load()
  lm = LanguageModel.load(TINY)
  handle = lm.device_handle(dev)
  stranger = LanguageModel(TINY)                                  # a fresh handle, uploaded nowhere
  assert lib.st_ctc_beam_stream_state_bytes(0, 0) == 0 and lib.st_ctc_beam_stream_state_bytes(129, 1) == 0
  up = lambda n: -(-n // 64) * 64                                 # header + 212 B per entry with a model, 40 B without; records of 64 B
  assert lib.st_ctc_beam_stream_state_bytes(64, 1) == up(32 + 64 * 212) and lib.st_ctc_beam_stream_state_bytes(65, 1) == up(32 + 128 * 212)
  assert lib.st_ctc_beam_stream_state_bytes(16, 0) == up(32 + 64 * 40)
  assert lib.st_ctc_beam_stream_pool_bytes(0, 16) == 0 and lib.st_ctc_beam_stream_pool_bytes(50, 100) >= 8 * 5001
  assert lib.st_ctc_beam_stream_ws(10) == 10 * 32 * 4 and lib.st_ctc_beam_stream_ws(0) == 0
  z = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device=dev)
  logits, rows, table = z(4 * 32, torch.float32), z(8), z(4)
  state, pool, ws, tail, result = z(32 + 128 * 212, torch.uint8), z(2 * 4096), z(4 * 32, torch.float32), z(64), z(4)
  ok = dict(logits=_ptr(logits), pitch=32, C=29, rows=_ptr(rows), table=_ptr(table), n_rows=4, S=1, beam=16, transform=0, lm=handle,
            w=(0.8, 0.0, 2.3, -1000.0), state=_ptr(state), pool=_ptr(pool), max_frames=16, ws=_ptr(ws), ws_bytes=4 * 32 * 4)

  def step(**kw):
    a = dict(ok, **kw)
    return lib.st_ctc_beam_stream_step(a['logits'], a['pitch'], a['C'], a['rows'], a['table'], a['n_rows'], a['S'], a['beam'], a['transform'],
                                       a['lm'], *_f(a['w']), a['state'], a['pool'], a['max_frames'], a['ws'], a['ws_bytes'], None)

  def read(**kw):
    a = dict(ok, tail=_ptr(tail), max_tail=64, result=_ptr(result))
    a.update(kw)
    return lib.st_ctc_beam_stream_read(a['table'], a['S'], a['beam'], a['lm'], *_f(a['w']), a['state'], a['pool'], a['max_frames'],
                                       a['tail'], a['max_tail'], a['result'], None)

  refused = [
      (step, dict(logits=None), 'null argument'), (step, dict(state=None), 'null argument'), (step, dict(pool=None), 'null argument'),
      (step, dict(table=None), 'null argument'), (step, dict(rows=None), 'null argument'),
      (step, dict(beam=0), 'beam width'), (step, dict(beam=129), 'beam width'),
      (step, dict(C=28), 'classes must be'), (step, dict(C=33, lm=None), 'classes'), (step, dict(C=1, lm=None), 'classes'),
      (step, dict(pitch=16), 'pitch'), (step, dict(transform=2), 'input_transform'),
      (step, dict(w=(float('nan'), 0.0, 2.3, -1000.0)), 'finite'), (step, dict(w=(0.8, 0.0, 2.3, float('inf'))), 'finite'),
      (step, dict(lm=stranger._handle), 'not on device'), (step, dict(ws_bytes=4 * 32 * 4 - 1), 'workspace'), (step, dict(ws=None), 'workspace'),
      (step, dict(max_frames=0), 'max_frames'), (step, dict(S=0), 'max_streams'), (step, dict(n_rows=-1), 'row count'),
      (read, dict(tail=None), 'null argument'), (read, dict(result=None), 'null argument'), (read, dict(state=None), 'null argument'),
      (read, dict(max_tail=0), 'max_tail'), (read, dict(beam=200), 'beam width'), (read, dict(w=(0.8, float('nan'), 2.3, -1000.0)), 'finite'),
      (read, dict(lm=stranger._handle), 'not on device'),
  ]
  with launch_trace() as tr:
    for fn, kw, text in refused:
      assert fn(**kw) != 0, kw
      assert text in lib.st_last_error().decode(), (kw, lib.st_last_error().decode())
  assert tr.lines == []
  torch.cuda.synchronize()


# ---- 3., 4a., 5. the layers above ------------------------------------------------------------------------------------------

SMALL = WL.w2l_layers(16, width=24, fc=40)


@pytest.fixture(scope='module')
def small(dev):
  from speecht_amd.engine import Wav2LetterEngine
  params = WL.xavier_params(SMALL, seed=7)
  params[-1] = (params[-1][0] * 12.0, params[-1][1] * 4.0)        # (peakier posteriors: the hypotheses are not all empty)
  eng = Wav2LetterEngine(SMALL, device=dev)
  eng.set_weights(params)
  return eng


def _beams():
  from speecht_amd.streaming import StreamBeam
  return {'free': lambda **kw: StreamBeam(beam_width=16, max_seconds=4.0, **kw),
          'lm': lambda **kw: StreamBeam(beam_width=16, lm=TINY, max_seconds=4.0, **kw)}


def _solo(eng, x, chunk, beam):
  """One stream alone: [(input frames, hyp, stable, logp)] after every step and after the finish, the greedy ids, the logits."""
  from speecht_amd.streaming import StreamingRecognizer
  rec = StreamingRecognizer(eng, 1, max_chunk_frames=64, beam=beam)
  slot = rec.open()
  seen, ids, rows = [], [], []
  for at in range(0, len(x), chunk):
    r = rec.step({slot: x[at:at + chunk]}, return_logits=True)
    ids += r.ids[slot]
    rows.append(r.logits[slot])
    if beam:
      seen.append((min(at + chunk, len(x)), r.hyp[slot], r.stable[slot], np.float32(r.logp[slot]).tobytes()))
  r = rec.finish(slot, return_logits=True)
  ids += r.ids[slot]
  rows.append(r.logits[slot])
  if beam:
    seen.append(('end', r.hyp[slot], r.stable[slot], np.float32(r.logp[slot]).tobytes()))
  return seen, ids, np.concatenate(rows), rec


@pytest.mark.parametrize('which', ['free', 'lm'])
def test_whole_path_two_chunkings(dev, small, which):
  from speecht_amd.language_model import LanguageModel
  make = _beams()[which]
  x = WL.synthetic_features(151, 151, 16).astype(np.float32)
  a, ids_a, logits, rec_a = _solo(small, x, 50, make())
  b, ids_b, logits_b, _ = _solo(small, x, 25, make())
  plain, ids_plain, logits_plain, rec_plain = _solo(small, x, 50, None)
  assert np.array_equal(logits, logits_b) and np.array_equal(logits, logits_plain)
  at = {k: v for k, *v in b}
  for k, *v in a:                                                 # hyp, stable and logp where both runs have a step boundary
    assert at[k] == v, k
  stables = [s for _, _, s, _ in a]
  assert all(p <= q for p, q in zip(stables, stables[1:])) and a[-1][2] == len(a[-1][1])
  # the final hypothesis is the whole-utterance search on the stream's own logits
  eng = _engine(dev, logits[:, None, :], [151 // 2])
  if which == 'lm':
    ref_ids, ref_lp = eng.lm_beam_search_decode(LanguageModel.load(TINY), 16)
  else:
    ref_ids, ref_lp = eng.beam_search_decode(16)
  assert a[-1][1] == ref_ids[0] and len(ref_ids[0]) > 0
  assert a[-1][3] == np.float32(ref_lp[0, 0]).tobytes()
  # beam=None: today's results and launches; with a beam the greedy ids stay, three launches come on top
  assert ids_plain == ids_a == ids_b and plain == []
  assert not hasattr(rec_plain, 'beam_state') and rec_plain._beam is None and rec_a.launches == rec_plain.launches + 3


def test_a_reopened_slot_starts_a_new_search(small):
  from speecht_amd.streaming import StreamingRecognizer
  make = _beams()['lm']
  x = WL.synthetic_features(31, 120, 16).astype(np.float32)
  y = WL.synthetic_features(32, 140, 16).astype(np.float32)
  solo_x, solo_y = _solo(small, x, 40, make())[0], _solo(small, y, 40, make())[0]
  rec = StreamingRecognizer(small, 2, max_chunk_frames=64, beam=make())
  a, b = rec.open(), rec.open()
  rec.step({a: y[:110], b: x[:40]})
  rec.close(a)                                                    # a's stream is dropped mid-way; its slot goes to y from the start
  a2 = rec.open()
  assert a2 == a
  got_x, got_y = [], []
  for k in range(1, 4):
    feeds = {a2: y[40 * (k - 1):40 * k]}
    if k < 3:
      feeds[b] = x[40 * k:40 * (k + 1)]
    r = rec.step(feeds)
    got_y.append((r.hyp[a2], r.stable[a2], np.float32(r.logp[a2]).tobytes()))
    if k < 3:
      got_x.append((r.hyp[b], r.stable[b], np.float32(r.logp[b]).tobytes()))
  r = rec.step({a2: y[120:]})
  got_y.append((r.hyp[a2], r.stable[a2], np.float32(r.logp[a2]).tobytes()))
  r = rec.finish_many([a2, b])
  got_y.append((r.hyp[a2], r.stable[a2], np.float32(r.logp[a2]).tobytes()))
  got_x.append((r.hyp[b], r.stable[b], np.float32(r.logp[b]).tobytes()))
  assert got_y == [tuple(v[1:]) for v in solo_y]
  assert got_x == [tuple(v[1:]) for v in solo_x[1:]]


def test_the_host_refuses_a_step_past_the_pool(small):
  from speecht_amd.streaming import StreamBeam, StreamError, StreamingRecognizer
  beam = lambda: StreamBeam(beam_width=16, max_seconds=0.32)      # 16 output frames
  x = WL.synthetic_features(33, 160, 16).astype(np.float32)
  y = WL.synthetic_features(34, 120, 16).astype(np.float32)      # 11 output frames before its finish, 60 with it
  rec = StreamingRecognizer(small, 2, max_chunk_frames=64, beam=beam())
  assert rec.max_frames == 16
  a, b = rec.open(), rec.open()
  first = rec.step({a: x[:130], b: y[:60]})                       # a: (130 - 99) // 2 + 1 = 16 frames: the pool is full
  assert rec._beam.frames[a] == 16
  launches = rec.launches
  from speecht_amd._lib import launch_trace
  with launch_trace() as tr:
    with pytest.raises(StreamError, match='node pool'):
      rec.step({a: x[130:132], b: y[60:120]})                     # a 17th frame: nothing of the step runs, b's part included
  assert tr.lines == [] and rec.launches == launches
  r = rec.step({b: y[60:120]})
  # b alone, same steps, same pool
  solo = StreamingRecognizer(small, 1, max_chunk_frames=64, beam=beam())
  s = solo.open()
  solo.step({s: y[:60]})
  q = solo.step({s: y[60:120]})
  assert (r.hyp[b], r.stable[b], r.logp[b], r.ids[b]) == (q.hyp[s], q.stable[s], q.logp[s], q.ids[s])
  with pytest.raises(StreamError, match='node pool'):
    rec.finish(b)                                                 # the flush would bring b to 60 frames


# ---- 5b. the command line ---------------------------------------------------------------------------------------------------

def test_cli_stream_with_a_language_model(dev, golden_dir, tmp_path, capsys, monkeypatch):
  import importlib.machinery
  import importlib.util
  from speecht_amd import transcription, vocabulary
  from speecht_amd.speech_input import SingleInputLoader
  from speecht_amd.speech_model import Session, Wav2LetterModel
  from speecht_amd.streaming import StreamBeam, stream_audio
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  loader = importlib.machinery.SourceFileLoader('speecht_cli_stream_beam_gpu', os.path.join(root, 'speecht-cli'))
  spec = importlib.util.spec_from_loader('speecht_cli_stream_beam_gpu', loader)
  cli = importlib.util.module_from_spec(spec)
  loader.exec_module(cli)
  flac = os.path.join(golden_dir, '1089-134686-0037.flac')
  samples, rate = transcription.load_native(flac)
  per = int(rate * 200 / 1000.0)
  pieces = [samples[at:at + per] for at in range(0, len(samples), per)]
  model = Wav2LetterModel(SingleInputLoader(128), 128, 29)       # a checkpoint written the way test_gpu_stream.py does
  model.add_training_ops()
  model.add_decoding_ops()
  model.finalize(str(tmp_path / 'log'), 'r', 'record')
  model.init_seed = 1234
  train = tmp_path / 'train'
  (train / 'run').mkdir(parents=True)
  partials = []
  with Session(dev) as sess:
    model.init_session(sess)
    model.saver.save(sess, str(train / 'run' / 'speechT'), global_step=model.global_step)
    beam = StreamBeam(beam_width=16, lm=TINY, max_seconds=len(samples) / float(rate) + 1.0)
    ids, _ = stream_audio(model.engine, pieces, rate, 128, 'running', lambda *a: partials.append(a), max_piece=per, beam=beam)
  cwd = tmp_path / 'cwd'
  cwd.mkdir()
  monkeypatch.chdir(cwd)
  capsys.readouterr()
  code = cli.main(['stream', '--train-dir', str(train), '--run-name', 'run', '--device', dev, '--beam-width', '16', '--language-model', TINY,
                   flac])
  lines = capsys.readouterr().out.splitlines()
  assert code == 0 and lines[-1] == '{}\t{}'.format(flac, vocabulary.ids_to_sentence(ids))
  fields = [l.split('\t') for l in lines[:-1]]
  assert len(fields) == len(partials) and all(len(f) == 3 for f in fields)
  final = [int(f[2]) for f in fields]
  assert all(p <= q for p, q in zip(final, final[1:]))
  for f, (seconds, hyp, stable) in zip(fields, partials):
    assert f[1] == vocabulary.ids_to_sentence(hyp) and int(f[2]) == stable and 0 <= stable <= len(hyp)
    assert lines[-1].split('\t', 1)[1].startswith(f[1][:int(f[2])])
  assert sorted(os.listdir(str(cwd))) == []
