"""Endpointing on the GPU, in the order the layers stack.
1. The endpoint kernel alone (st_ctc_greedy_endpoint_stream): every step's events, pieces, ids and carried state equal the host form
   bit for bit and the specification (tests/endpoint_oracle.py), for every way of cutting the rows; every final's greedy ids and sum
   equal st_ctc_greedy_decode on the utterance's rows alone; nothing is written behind the outputs.
2. Composed with st_ctc_beam_stream_step_pieces: every final equals the whole-utterance search on its rows -- ids, length and the
   log-probability's bits -- whatever the cut, on a node pool of M frames that is never overrun and never full.
3. StreamingRecognizer(endpoint=...): the logits do not change, the finals are the specification's segments of those logits decoded
   offline, for two chunkings and beside a second stream; slots are reused; endpoint=None launches what it launched before."""
import ctypes

import numpy as np
import pytest

from tests import endpoint_cases as EC
from tests import endpoint_oracle as EO
from tests.test_gpu_lm_beam import TINY, _engine

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A5A5A5A5A
WEIGHTS = (0.8, 0.0, 2.3, -1000.0)
GUARD = 16


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def _ptr(t):
  return ctypes.c_void_p(t.data_ptr())


class DeviceStep:
  """`step_fn` of tests.endpoint_cases.drive on the kernel.  State and score start as a pattern (the first step resets), every output is
  pre-filled, and guard words lie behind ids, events and pieces.  The same step also runs through the host form on a state of its
  own: all outputs must be equal bit for bit.  The step's device buffers stay for what is stacked on top (the beam searches)."""

  def __init__(self, dev, C, space_id, R, L, M, S):
    from speecht_amd import _lib
    self.lib, self.dev, self.S = _lib, dev, S
    self.args = (C, space_id, R, L, M)
    self.state = torch.full((S * 8,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    self.score = torch.full((S * 256,), 1e30, dtype=torch.float32, device=dev)
    self.host = EC.host_step_fn(_lib.load(), C, space_id, R, L, M, S)

  def __call__(self, buf, rows, table, max_rows, P):
    C, space_id, R, L, M = self.args
    S, dev = self.S, self.dev
    fill = lambda n: torch.full((n + GUARD,), -77, dtype=torch.int32, device=dev)
    self.buf, self.rows, self.table = torch.from_numpy(buf).to(dev), torch.from_numpy(rows).to(dev), torch.from_numpy(table).to(dev)
    self.n_rows = int(table[:, 1].sum())
    ids, events, self.pieces = fill(S * max_rows), fill(S * P * 8), fill(P * S * 4)
    new_count = torch.full((S,), -77, dtype=torch.int32, device=dev)
    neg_sum = torch.full((S,), float('nan'), dtype=torch.float32, device=dev)
    self.lib.call('st_ctc_greedy_endpoint_stream', _ptr(self.buf), EC.PITCH, C, _ptr(self.rows), _ptr(self.table), S, space_id, R, L, M, max_rows,
                  _ptr(self.state), _ptr(self.score), _ptr(ids), max_rows, _ptr(new_count), _ptr(neg_sum), _ptr(events), _ptr(self.pieces), P,
                  None)
    torch.cuda.synchronize()
    ids, events, pieces = ids.cpu().numpy(), events.cpu().numpy(), self.pieces.cpu().numpy()
    assert (ids[S * max_rows:] == -77).all() and (events[S * P * 8:] == -77).all() and (pieces[P * S * 4:] == -77).all()
    out = EC.Outputs(self.state.cpu().numpy().reshape(S, 8), ids[:S * max_rows].reshape(S, max_rows), new_count.cpu().numpy(),
                     neg_sum.cpu().numpy(), events[:S * P * 8].reshape(S, P, 8), pieces[:P * S * 4].reshape(P, S, 4))
    ref = self.host(buf, rows, table, max_rows, P)
    live = table[:, 3] != 0                                         # streams whose record has been reset: the others' is still the pattern
    self.live = live if not hasattr(self, 'live') else (self.live | live)
    for s in np.flatnonzero(self.live):
      n = int(ref.new_count[s])
      assert out.new_count[s] == n and (out.ids[s, :n] == ref.ids[s, :n]).all() and (out.ids[s, n:] == -77).all(), s
      assert out.neg_sum[s].tobytes() == ref.neg_sum[s].tobytes(), s
      assert (out.state[s] == ref.state[s]).all() and (out.pieces[:, s] == ref.pieces[:, s]).all(), s
      used = [int(e[0]) for e in ref.events[s]].index(0) + 1 if 0 in ref.events[s, :, 0] else P
      assert (out.events[s, :used] == ref.events[s, :used]).all() and (out.events[s, used:] == -77).all(), s
    return out


def _offline_batch(dev, slices, C):
  """[rows_i, C] slices -> an engine holding them as one batch [T, B, C], and their lengths."""
  T = max([len(x) for x in slices] + [1])
  batch = np.zeros((T, len(slices), C), np.float32)
  for i, x in enumerate(slices):
    batch[:len(x), i] = x
  lens = [len(x) for x in slices]
  return _engine(dev, batch, lens), lens


# ---- 1. the endpoint kernel alone -------------------------------------------------------------------------------------------------

KERNEL_CASES = EC.sweep()[::13]


@pytest.mark.parametrize('case', KERNEL_CASES, ids=lambda c: 'S{}-C{}-sp{}-R{}-L{}-M{}'.format(*c[1:]))
def test_kernel_equals_the_host_form_and_the_specification(dev, case):
  from speecht_amd._lib import launch_trace
  seed, S, C, space_id, R, L, M = case
  logits, lens = EC.make_streams(seed, S, C, space_id, R, L, M)
  plans = EC.cut_plans(S)
  slices, want = [], []
  for i in (5, seed % 5):                                           # the cuts dealt round the streams, and one cut for all
    with launch_trace() as tr:
      seen, finals, specs = EC.drive(DeviceStep(dev, C, space_id, R, L, M, S), logits, lens, C, space_id, R, L, M, plans[i],
                                     sit_out=i == 5, finish_apart=(0,) if i == 5 else ())
    assert tr.lines and all(l.startswith('ctc_greedy_endpoint_stream ') for l in tr.lines)
    assert sum(seen[kind] for kind in (1, 2, 3, 4)) > 0
    for s in range(S):
      for f in finals[s]:
        slices.append(logits[s][f['event'][1]:f['event'][2]])
        want.append((f['ids'], f['event'][6]))
  # the greedy decoder on each utterance's rows alone: the same ids, the same sum
  eng, _ = _offline_batch(dev, slices, C)
  ids, neg = eng.greedy_decode()
  assert len(want) > 0 and ids == [w[0] for w in want]
  assert neg.astype(np.float32).reshape(-1).view(np.int32).tolist() == [w[1] for w in want]


def test_kernel_meets_every_situation(dev):
  """Over a few cases with small parameters: events on a step's first and last row, two in a step, every way of finishing."""
  total = {}
  for seed, S, C, space_id, R, L, M in [c for c in EC.sweep() if c[4:] == (1, 3, 9) or c[4:] == (2, 1, 9)][:6]:
    logits, lens = EC.make_streams(seed, S, C, space_id, R, L, M, T=60)
    for i, cuts in enumerate(([2] * S, [7] * S, [10] * S)):
      seen, _, _ = EC.drive(DeviceStep(dev, C, space_id, R, L, M, S), logits, lens, C, space_id, R, L, M, cuts, sit_out=i == 0,
                            finish_apart=(0,) if i < 2 else ())
      for key, n in seen.items():
        total[key] = total.get(key, 0) + n
  assert all(total[name] > 0 for name in EC.SITUATIONS) and all(total[k] > 0 for k in (1, 2, 3, 4)), total


def test_kernel_refuses_bad_requests_without_a_launch(dev):
  from speecht_amd import _lib
  from speecht_amd._lib import launch_trace
  lib = _lib.load()
  z = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device=dev)
  buf, rows, table, state, score = z(4 * 32, torch.float32), z(8), z(4), z(8), z(256, torch.float32)
  ids, count, neg, events, pieces = z(8), z(1), z(1, torch.float32), z(4 * 8), z(4 * 4)
  ok = dict(C=29, space=27, R=2, L=3, M=9, max_rows=4, P=4, pieces=_ptr(pieces))

  def run(**kw):
    a = dict(ok, **kw)
    return lib.st_ctc_greedy_endpoint_stream(_ptr(buf), 32, a['C'], _ptr(rows), _ptr(table), 1, a['space'], a['R'], a['L'], a['M'], a['max_rows'],
                                             _ptr(state), _ptr(score), _ptr(ids), 8, _ptr(count), _ptr(neg), _ptr(events), a['pieces'], a['P'],
                                             None)

  with launch_trace() as tr:
    for kw, text in ((dict(R=0), 'silence_frames'), (dict(L=0), 'lead_frames'), (dict(M=2), 'below lead_frames'), (dict(space=29), 'space_id'),
                     (dict(P=2), 'pieces'), (dict(max_rows=0), 'max_rows'), (dict(C=65), 'classes'), (dict(pieces=None), 'null')):
      assert run(**kw) != 0, kw
      assert text in lib.st_last_error().decode(), (kw, lib.st_last_error().decode())
  assert tr.lines == []
  torch.cuda.synchronize()


# ---- 2. the beam searches behind the endpointer -----------------------------------------------------------------------------------

class PiecesSearch:
  """The searches of S streams behind a `DeviceStep`: st_ctc_beam_stream_step_pieces on the pieces the endpoint kernel left on the
  device, the host's part of the contract as `StreamingRecognizer` plays it -- pieces in order, a reset piece starts from an empty
  hypothesis, a read appends the reported tail above the stable length, a piece with a limit is a final.  State and pool start as a
  pattern; the pool holds M frames and lies inside a larger tensor whose tail must keep the pattern."""

  def __init__(self, dev, step, S, C, M, beam, lm, transform, max_tail=64):
    from speecht_amd import _lib
    self.lib, raw = _lib, _lib.load()
    self.dev, self.step, self.S, self.C, self.M, self.beam, self.transform, self.max_tail = dev, step, S, C, M, beam, transform, max_tail
    self.handle = lm.device_handle(dev) if lm is not None else None
    self.state_bytes = int(raw.st_ctc_beam_stream_state_bytes(beam, int(lm is not None)))
    self.pool_bytes = int(raw.st_ctc_beam_stream_pool_bytes(M, beam))
    self.state = torch.full((S * self.state_bytes // 8,), PATTERN, dtype=torch.int64, device=dev)
    self.pool = torch.full((S * self.pool_bytes // 8 + 64,), PATTERN, dtype=torch.int64, device=dev)
    self.hyp, self.stable = [[] for _ in range(S)], [0] * S
    self.finals = [[] for _ in range(S)]
    self.statuses = set()

  def on_step(self, k, plan, out, table):
    S, P, mt = self.S, out.pieces.shape[0], self.max_tail
    n_rows = self.step.n_rows
    ws_bytes = max(n_rows, 1) * 32 * 4
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=self.dev)
    tail = torch.full((P * S * mt + GUARD,), -77, dtype=torch.int32, device=self.dev)
    result = torch.full((P * S * 4 + GUARD,), -77, dtype=torch.int32, device=self.dev)
    self.lib.call('st_ctc_beam_stream_step_pieces', _ptr(self.step.buf), EC.PITCH, self.C, _ptr(self.step.rows), _ptr(self.step.pieces), P,
                  n_rows, S, self.beam, self.transform, self.handle, *[ctypes.c_float(w) for w in WEIGHTS], _ptr(self.state), _ptr(self.pool),
                  self.M, _ptr(ws), ws_bytes, _ptr(tail), mt, _ptr(result), None)
    torch.cuda.synchronize()
    tail, result = tail.cpu().numpy(), result.cpu().numpy()
    assert (tail[P * S * mt:] == -77).all() and (result[P * S * 4:] == -77).all()
    tail, result = tail[:P * S * mt].reshape(P, S, mt), result[:P * S * 4].reshape(P, S, 4)
    for s in plan:
      closing = iter([e for e in out.events[s].tolist() if e[0] in EO.FINAL_KINDS][:P])
      for p in range(P):
        first, rows, limit, reset = out.pieces[p, s].tolist()
        if rows == 0 and limit < 0 and not reset:
          assert (result[p, s] == -77).all()                        # an unused slot: the read-out left at once
          continue
        if reset:
          self.hyp[s], self.stable[s] = [], 0
        length, stable, status = int(result[p, s, 0]), int(result[p, s, 1]), int(result[p, s, 3])
        self.statuses.add(status)
        assert 0 <= length - self.stable[s] <= mt, (k, s, p, length, self.stable[s])
        self.hyp[s] = self.hyp[s][:self.stable[s]] + tail[p, s, :length - self.stable[s]].tolist()
        self.stable[s] = stable
        if limit >= 0:
          e = next(closing)
          assert e[2] == limit
          self.finals[s].append((e[1], e[2], list(self.hyp[s]), int(result[p, s, 2])))
          self.hyp[s], self.stable[s] = [], 0

  def pattern_intact(self):
    return bool((self.pool[self.S * self.pool_bytes // 8:] == PATTERN).all())


SEARCH_PARAMS = {'lm': (29, 27, 3, 5, 24), 'free': (5, -1, 2, 3, 9)}


@pytest.mark.parametrize('transform', [0, 1])
@pytest.mark.parametrize('kind', ['free', 'lm'])
@pytest.mark.parametrize('beam', [1, 4, 16, 100, 128])
def test_finals_equal_the_whole_utterance_search_for_every_cut(dev, beam, kind, transform):
  from speecht_amd._lib import launch_trace
  from speecht_amd.language_model import LanguageModel
  C, space_id, R, L, M = SEARCH_PARAMS[kind]
  S, T = 3, 90
  lm = LanguageModel.load(TINY) if kind == 'lm' else None
  logits, lens = EC.make_streams(beam + transform, S, C, space_id, R, L, M, T=T)
  lens[2] = T - 3                                                   # (no empty stream here: three streams that decode)
  runs = []
  for cuts in ([7, 10, 80], [80, 1, 2], [10] * 3):
    step = DeviceStep(dev, C, space_id, R, L, M, S)
    search = PiecesSearch(dev, step, S, C, M, beam, lm, transform)
    with launch_trace() as tr:
      seen, finals, specs = EC.drive(step, logits, lens, C, space_id, R, L, M, cuts, on_step=search.on_step)
    want = 'ctc_beam_stream_lm<' if lm is not None else 'ctc_beam_stream<'
    assert sum(l.startswith(want) for l in tr.lines) == sum(l.startswith('ctc_beam_stream_read<') for l in tr.lines) > 0
    assert search.statuses == {0} and search.pattern_intact()       # the pool of M frames is never full, nothing lands behind it
    assert [[(u0, end) for u0, end, _, _ in search.finals[s]] for s in range(S)] == [[e[1:3] for e in specs[s].finals()] for s in range(S)]
    assert seen[1] >= 2 and seen[2] >= 1 and seen[3] >= 1 and seen[4] >= 1, seen
    runs.append(search.finals)
  assert runs[1] == runs[0] and runs[2] == runs[0]                  # the same finals, bit for bit, for every cut
  flat = [f for s in range(S) for f in runs[0][s]]
  eng, _ = _offline_batch(dev, [logits[s][u0:end] for s in range(S) for u0, end, _, _ in runs[0][s]], C)
  name = 'log10_softmax' if transform else None
  ref_ids, ref_lp = eng.beam_search_decode(beam, name) if lm is None else eng.lm_beam_search_decode(lm, beam, name, *WEIGHTS)
  assert [f[2] for f in flat] == ref_ids
  assert [f[3] for f in flat] == np.asarray(ref_lp, np.float32).reshape(-1).view(np.int32).tolist()
  assert any(len(f[2]) > 0 for f in flat) and any(f[1] - f[0] == M for f in flat)      # (some text, and an utterance that fills the pool)


# ---- 3. the recogniser ------------------------------------------------------------------------------------------------------------

RLM = (8, 20, 40)            # EC.RECOGNIZER_SECONDS at 20 ms per row


@pytest.fixture(scope='module')
def tiny(dev):
  from speecht_amd.engine import Wav2LetterEngine
  layers, params = EC.recognizer_model()
  eng = Wav2LetterEngine(layers, device=dev)
  eng.set_weights(params)
  return eng


def _beam(which, max_seconds=1.0):
  """(With endpointing ``max_seconds`` must not matter: one second would not hold these streams.)"""
  from speecht_amd.streaming import StreamBeam
  if which == 'greedy':
    return None
  return StreamBeam(beam_width=16, lm=TINY if which == 'lm' else None, max_seconds=max_seconds)


def _endpointing():
  from speecht_amd.streaming import Endpointing
  return Endpointing(**EC.RECOGNIZER_SECONDS)


def _key(u):
  return (u.index, u.kind, u.start_frame, u.end_frame, u.first_speech, u.last_speech, tuple(u.ids), tuple(u.greedy_ids),
          None if u.logp is None else np.float32(u.logp).tobytes(), np.float32(u.score).tobytes())


def _stream(rec, slot, x, chunk, others=None):
  """Feed ``x`` in chunks of ``chunk`` frames and finish -> (finals, logits rows, the open hypotheses seen).  ``others``: {slot: (x, chunk)}
  fed beside it, each at its own pace, and finished in a step of their own; their finals come back too."""
  finals, rows, seen = [], [], []
  side = {s: dict(x=xs, chunk=c, at=0, finals=[], rows=[]) for s, (xs, c) in (others or {}).items()}
  for at in range(0, len(x), chunk):
    feeds = {slot: x[at:at + chunk]}
    for s, o in side.items():
      if o['at'] < len(o['x']) and (at // chunk) % 3 != 2:          # (the others sit every third step out)
        feeds[s] = o['x'][o['at']:o['at'] + o['chunk']]
        o['at'] += o['chunk']
    r = rec.step(feeds, return_logits=True)
    finals += r.finals[slot]
    rows.append(r.logits[slot])
    seen.append((list(r.hyp.get(slot, r.open_ids[slot])), r.stable.get(slot)))
    for s, o in side.items():
      if s in feeds:
        o['finals'] += r.finals[s]
        o['rows'].append(r.logits[s])
  r = rec.finish(slot, return_logits=True)
  finals += r.finals[slot]
  rows.append(r.logits[slot])
  assert r.open_ids[slot] == [] and r.hyp.get(slot, []) == []       # the end of the stream closes what was open
  for s, o in side.items():
    while o['at'] < len(o['x']):
      r = rec.step({s: o['x'][o['at']:o['at'] + o['chunk']]}, return_logits=True)
      o['at'] += o['chunk']
      o['finals'] += r.finals[s]
      o['rows'].append(r.logits[s])
    r = rec.finish(s, return_logits=True)
    o['finals'] += r.finals[s]
    o['rows'].append(r.logits[s])
  return finals, np.concatenate(rows), seen, {s: (o['finals'], np.concatenate(o['rows'])) for s, o in side.items()}


def _check_against_offline(dev, which, finals, logits, n_input):
  """The finals are the specification's segments of the stream's own logits, each decoded offline on its rows alone."""
  from speecht_amd.language_model import LanguageModel
  spec = EO.Spec(logits, 29, 27, *RLM, limit=n_input // 2)
  kinds = {1: 'silence', 2: 'length', 4: 'end'}
  assert [(u.index, u.kind, u.start_frame, u.end_frame, u.first_speech, u.last_speech) for u in finals] == \
      [(e[5], kinds[e[0]], e[1], e[2], e[3], e[4]) for e in spec.finals()]
  count = lambda kind: sum(1 for e in spec.events if e[0] == kind)
  assert count(1) >= 2 and count(2) >= 1 and count(3) >= 1, [count(k) for k in (1, 2, 3, 4)]   # the device's own logits hold every event
  eng, _ = _offline_batch(dev, [logits[u.start_frame:u.end_frame] for u in finals], 29)
  ids, neg = eng.greedy_decode()
  assert [u.greedy_ids for u in finals] == ids
  assert [np.float32(u.score).tobytes() for u in finals] == [np.float32(v).tobytes() for v in neg.reshape(-1)]
  if which == 'greedy':
    assert all(u.ids == u.greedy_ids and u.logp is None for u in finals)
    return
  ref_ids, ref_lp = eng.beam_search_decode(16) if which == 'free' else eng.lm_beam_search_decode(LanguageModel.load(TINY), 16)
  assert [u.ids for u in finals] == ref_ids and any(len(u.ids) > 0 for u in finals)
  assert [np.float32(u.logp).tobytes() for u in finals] == [np.float32(v).tobytes() for v in np.asarray(ref_lp).reshape(-1)]


@pytest.mark.parametrize('which', ['greedy', 'free', 'lm'])
def test_recognizer_finals_are_offline_decodes_of_the_specification_s_segments(dev, tiny, which):
  from speecht_amd._lib import launch_trace
  from speecht_amd.streaming import StreamingRecognizer
  xa, xb = EC.recognizer_features('a'), EC.recognizer_features('b')
  plain = StreamingRecognizer(tiny, 1, max_chunk_frames=64)
  slot = plain.open()
  rows = [plain.step({slot: xa[at:at + 50]}, return_logits=True).logits[slot] for at in range(0, len(xa), 50)]
  rows.append(plain.finish(slot, return_logits=True).logits[slot])
  logits_plain = np.concatenate(rows)
  # alone, two chunkings
  rec = StreamingRecognizer(tiny, 1, max_chunk_frames=64, beam=_beam(which), endpoint=_endpointing())
  with launch_trace() as tr:
    finals, logits, seen, _ = _stream(rec, rec.open(), xa, 50)
  assert any(l.startswith('ctc_greedy_endpoint_stream ') for l in tr.lines)
  assert logits.tobytes() == logits_plain.tobytes()                 # endpointing never touches the forward pass
  _check_against_offline(dev, which, finals, logits, len(xa))
  assert any(hyp for hyp, _ in seen)                                # (the partials show the open utterance)
  rec2 = StreamingRecognizer(tiny, 1, max_chunk_frames=64, beam=_beam(which), endpoint=_endpointing())
  finals2, logits2, _, _ = _stream(rec2, rec2.open(), xa, 37)
  assert logits2.tobytes() == logits.tobytes() and [_key(u) for u in finals2] == [_key(u) for u in finals]
  # beside a second stream that goes at its own pace
  duo = StreamingRecognizer(tiny, 2, max_chunk_frames=64, beam=_beam(which), endpoint=_endpointing())
  a, b = duo.open(), duo.open()
  finals3, logits3, _, side = _stream(duo, a, xa, 50, others={b: (xb, 64)})
  assert logits3.tobytes() == logits.tobytes() and [_key(u) for u in finals3] == [_key(u) for u in finals]
  finals_b, logits_b = side[b]
  spec_b = EO.Spec(logits_b, 29, 27, *RLM, limit=len(xb) // 2)
  assert [(u.start_frame, u.end_frame) for u in finals_b] == [e[1:3] for e in spec_b.finals()] and finals_b[-1].kind == 'end'


def test_recognizer_reuses_slots_and_refuses_a_blind_step(dev, tiny):
  from speecht_amd.streaming import StreamError, StreamingRecognizer
  xa, xb = EC.recognizer_features('a')[:900], EC.recognizer_features('b')
  solo = StreamingRecognizer(tiny, 1, max_chunk_frames=64, beam=_beam('free'), endpoint=_endpointing())
  want, _, _, _ = _stream(solo, solo.open(), xa, 60)
  rec = StreamingRecognizer(tiny, 2, max_chunk_frames=64, beam=_beam('free'), endpoint=_endpointing())
  a, b = rec.open(), rec.open()
  rec.step({a: xb[:260], b: xb[:64]})                               # a's stream is dropped inside an utterance ...
  rec.close(a)
  again = rec.open()
  assert again == a
  got, _, _, _ = _stream(rec, again, xa, 60)                        # ... and its slot starts the next stream from nothing
  assert len(want) >= 2 and [_key(u) for u in got] == [_key(u) for u in want]
  with pytest.raises(StreamError, match='fetch=False'):
    rec.step({b: xb[64:128]}, fetch=False)
  with pytest.raises(StreamError):
    StreamingRecognizer(tiny, 1, endpoint=_endpointing()).step({0: xb[:10]}, fetch=False)


def test_cli_stream_with_endpointing(dev, golden_dir, tmp_path, capsys, monkeypatch):
  """`speecht-cli stream --endpoint` prints what `stream_audio(endpoint=...)` reports: a line per final as it closes, the partials of the
  open utterance, the finals joined at the end."""
  import importlib.machinery
  import importlib.util
  import os
  from speecht_amd import transcription, vocabulary
  from speecht_amd.speech_input import SingleInputLoader
  from speecht_amd.speech_model import Session, Wav2LetterModel
  from speecht_amd.streaming import Endpointing, stream_audio
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  loader = importlib.machinery.SourceFileLoader('speecht_cli_endpoint_gpu', os.path.join(root, 'speecht-cli'))
  spec = importlib.util.spec_from_loader('speecht_cli_endpoint_gpu', loader)
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
  said = []
  settings = dict(silence=0.1, lead=0.3, max_utterance=1.5)       # short enough for several utterances in the file
  with Session(dev) as sess:
    model.init_session(sess)
    model.saver.save(sess, str(train / 'run' / 'speechT'), global_step=model.global_step)
    finals, seconds = stream_audio(model.engine, pieces, rate, 128, 'running', lambda *a: said.append(('partial',) + a), max_piece=per,
                                   endpoint=Endpointing(**settings), on_final=lambda u: said.append(('final', u)))
  assert len(finals) >= 2 and [u.index for u in finals] == list(range(len(finals))) and finals[-1].end_frame <= len(samples) // 160 // 2 + 1
  cwd = tmp_path / 'cwd'
  cwd.mkdir()
  monkeypatch.chdir(cwd)
  capsys.readouterr()
  code = cli.main(['stream', '--train-dir', str(train), '--run-name', 'run', '--device', dev, '--endpoint', '--endpoint-silence', '0.1',
                   '--endpoint-lead', '0.3', '--max-utterance', '1.5', flac])
  lines = capsys.readouterr().out.splitlines()
  assert code == 0 and lines[-1] == '{}\t{}'.format(flac, ' '.join(vocabulary.ids_to_sentence(u.ids) for u in finals))
  assert len(lines) - 1 == len(said)
  for line, item in zip(lines, said):
    f = line.split('\t')
    if item[0] == 'final':
      u = item[1]
      assert f == ['utt', str(u.index), '{:.2f}'.format(u.first_speech * 0.02), '{:.2f}'.format((u.last_speech + 1) * 0.02),
                   vocabulary.ids_to_sentence(u.ids)]
      assert u.start_frame <= u.first_speech <= u.last_speech < u.end_frame
    else:
      assert f == ['{:.2f}'.format(item[1]), vocabulary.ids_to_sentence(item[2])]
  assert sorted(os.listdir(str(cwd))) == []


def test_without_endpointing_the_launches_are_the_old_ones(dev, tiny):
  from speecht_amd._lib import launch_trace
  from speecht_amd.streaming import StreamingRecognizer
  x = EC.recognizer_features('b')[:200]
  for which, decoders in (('greedy', []), ('lm', ['ctc_beam_stream_lm<', 'ctc_beam_stream_read<'])):
    rec = StreamingRecognizer(tiny, 1, max_chunk_frames=64, beam=_beam(which, 10.0))
    assert rec.endpoint is None and not hasattr(rec, 'ep_state') and rec._endpoint is None and rec.n_pieces == 1
    slot = rec.open()
    rec.step({slot: x[:150]})
    with launch_trace() as tr:
      rec.step({slot: x[150:]})
    names = [l.split(' ')[0].split('<')[0] + ('<' if '<' in l.split(' ')[0] else '') for l in tr.lines]
    assert names == ['stream_conv<'] * 11 + decoders, tr.lines
    assert rec.launches == 1 + 22 + 2 + (3 if decoders else 0)      # feed, products with epilogues, advance + greedy, search + log-softmax + read
    assert rec.dec_out.numel() == 1 * rec.max_new + 2 + (4 + 256 if decoders else 0)
