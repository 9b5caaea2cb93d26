"""N-best lists for the finals of live streams (st_ctc_beam_stream_read_nbest / _step_pieces_nbest, StreamBeam(nbest=, rescore=),
`speecht-cli stream --nbest`): however a stream's rows are cut, a finishing read-out leaves in the arena the list the whole-utterance
N-best searches return on the same rows -- ids, lengths, log-probability bits, the number of hypotheses -- while `result` and `tail`
stay what st_ctc_beam_stream_read writes; open streams write nothing; an arena that is too small loses whole lists and nothing else;
endpointed pieces; the recogniser's lists, their rescoring and the words of the re-ranked ids; nbest=None launches what it launched."""
import ctypes
import importlib.machinery
import importlib.util
import os

import numpy as np
import pytest

from tests import stream_beam_cases as SC
from tests import stream_hotword_cases as HC
from tests.test_gpu_lm_beam import TINY, _engine, _model
from tests.test_gpu_stream_hotwords import Harness, _sets

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTS = (1, 2, 7, 10, 80)
WEIGHTS = (0.8, 0.0, 2.3, -1000.0)
FILL = 0x5A5A5A5A                                               # no header: its sixth word is 0
GUARD = 64


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def _ptr(t):
  return ctypes.c_void_p(t.data_ptr())


def _f(values):
  return [ctypes.c_float(v) for v in values]


class ListHarness(Harness):
  """The harness of tests/test_gpu_stream_hotwords.py (biased with ``sets``, unbiased without) reading through
  st_ctc_beam_stream_read_nbest.  Every read first runs st_ctc_beam_stream_read (or _read_bias) on a COPY of the records into copies of
  the outputs: records, `result` and `tail` must come out the same, byte for byte.  The arena lies inside a larger tensor whose tail holds
  the fill pattern, the counter starts as garbage (the entry point zeroes it).  ``lists[s]``: the list stream s's finishing read left."""

  def __init__(self, dev, logits, lens, beam, n_best, lm=None, transform=0, sets=None, which=None, arena_words=None, **kw):
    super().__init__(dev, logits, lens, beam, lm, transform, sets, which, max_frames=80, **kw)
    self.n_best = n_best
    self.cap = self.S * (6 + n_best * (2 + self.T)) if arena_words is None else arena_words
    self.arena = torch.full((self.cap + GUARD,), FILL, dtype=torch.int32, device=dev)
    self.used = torch.full((1,), 123456, dtype=torch.int32, device=dev)
    self.lists, self.demand, self.records, self.raw_arena, self.reads = {}, 0, {}, None, 0

  def read(self, d_table, biased=None):
    from speecht_amd import nbest
    biased = bool(self.bias)
    state2, tail2, result2 = self.state.clone(), self.tail.clone(), self.result.clone()
    self.lib.call('st_ctc_beam_stream_read' + ('_bias' if biased else ''), _ptr(d_table), self.S, self.beam, self.handle, *_f(self.weights),
                  _ptr(state2), _ptr(self.pool), self.max_frames, _ptr(tail2), self.max_tail, _ptr(result2), None, *self.bias)
    self.lib.call('st_ctc_beam_stream_read_nbest', _ptr(d_table), self.S, self.beam, self.handle, *_f(self.weights), _ptr(self.state),
                  _ptr(self.pool), self.max_frames, _ptr(self.tail), self.max_tail, _ptr(self.result), None, *(self.bias or (None, None)),
                  self.n_best, _ptr(self.arena), self.cap, _ptr(self.used))
    torch.cuda.synchronize()
    assert torch.equal(tail2, self.tail) and torch.equal(result2, self.result) and torch.equal(state2, self.state)
    table = d_table.cpu().numpy()
    arena, used = self.arena.cpu().numpy(), int(self.used.item())
    assert (arena[self.cap:] == FILL).all()                        # the words behind the arena
    finishing = [s for s in range(self.S) if table[s, 2] >= 0]
    self.reads += 1
    self.demand, self.raw_arena = used, arena[:self.cap].copy()
    lists, lost = nbest.read_arena(arena[:self.cap], used, {(0, s): self.hyp[s][:self.stable[s]] for s in finishing})
    if not finishing:
      assert used == 0 and (arena == FILL).all()                   # open streams write nothing
    if used <= self.cap:
      assert lost == 0 and sorted(lists) == [(0, s) for s in finishing]
      assert (arena[used:] == FILL).all()
    self.records = lists
    for (_, s), hyps in lists.items():
      self.lists[s] = [(h['ids'], np.float32(h['log_prob']).tobytes()) for h in hyps]
    self.arena.fill_(FILL)
    res, tail = self.result.cpu().numpy().reshape(self.S, 4), self.tail.cpu().numpy().reshape(self.S, self.max_tail)
    for s in range(self.S):                                        # the host's part, as in the parent harness
      if table[s, 1] > 0 or table[s, 2] >= 0 or table[s, 3]:
        length, old = int(res[s, 0]), self.stable[s]
        self.status[s] = int(res[s, 3])
        self.logp[s] = res[s, 2:3].view(np.float32)[0]
        assert 0 <= length - old <= self.max_tail, (s, length, old)
        self.hyp[s] = self.hyp[s][:old] + tail[s, :length - old].tolist()
        self.stable[s] = int(res[s, 1])


def _offline_lists(eng, n_best, beam, lm, transform, hw=None, weights=WEIGHTS):
  name = 'log10_softmax' if transform else None
  if lm is None:
    lists = eng.beam_search_decode_nbest(n_best, beam, name, hotwords=hw)
  else:
    lists = eng.lm_beam_search_decode_nbest(lm, n_best, beam, name, *weights, hotwords=hw)
  return [[(list(ids), np.float32(lp).tobytes()) for ids, lp in hyps] for hyps in lists]


def _inputs(kind, beam):
  if kind == 'free5':
    return SC.cases5(beam)
  return SC.cases29(10 * beam + (int(kind) if kind != 'free' else 0))


def _check_run(h, want, ids, lp):
  """The lists against the offline search's, hypothesis 0 against the top path the read-out reported."""
  for s in range(h.S):
    assert h.lists[s] == want[s], (s, h.lists[s][:2], want[s][:2])
    assert [len(i) for i, _ in h.lists[s]] == [len(i) for i, _ in want[s]]
    assert h.lists[s][0] == (ids[s], np.float32(lp[s]).tobytes())
  assert h.status == [0] * h.S and h.pattern_intact()


# ---- 1. every cut returns the offline N-best search ------------------------------------------------------------------------------

@pytest.mark.parametrize('transform', [0, 1])
@pytest.mark.parametrize('kind', ['free', 'free5', '1', '3', '5'])
@pytest.mark.parametrize('beam', [1, 16, 64, 100, 128])
def test_every_cut_returns_the_offline_nbest_search_bit_for_bit(dev, tmp_path_factory, beam, kind, transform):
  from speecht_amd._lib import launch_trace
  logits, lens = _inputs(kind, beam)
  lm = _model(str(tmp_path_factory.getbasetemp()), int(kind))[0] if kind.isdigit() else None
  eng = _engine(dev, logits, lens)
  longest = 0
  for k, n_best in enumerate(sorted({1, min(3, beam), beam})):
    want = _offline_lists(eng, n_best, beam, lm, transform)
    cuts = [CUTS[(s + 2 * k) % len(CUTS)] for s in range(len(lens))]   # the streams side by side, each with another cut
    h = ListHarness(dev, logits, lens, beam, n_best, lm, transform)
    with launch_trace() as tr:
      ids, lp = h.run(cuts)
    reads = [l for l in tr.lines if l.startswith('ctc_beam_stream_read_nbest<' + ('wide' if beam > 64 else 'wave'))]
    assert len(reads) == h.reads and all('n_best={} '.format(n_best) in l for l in reads), tr.lines[:4]
    _check_run(h, want, ids, lp)
    assert [len(h.lists[s]) for s in range(h.S)] == [len(w) for w in want] and all(len(w) <= n_best for w in want)
    assert len(want[3]) == 1 and want[3][0][0] == [] and len(want[4]) <= min(n_best, logits.shape[2])   # lengths 0 and 1: short lists
    longest = max([longest] + [len(l) for l in h.lists.values()])
  if beam > 64:
    assert longest > 64                                             # the second round of the chain walk ran


# ---- 2. biased searches ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('with_lm', [False, True])
@pytest.mark.parametrize('beam', [16, 100])
def test_biased_lists_equal_the_offline_biased_search(dev, beam, with_lm):
  from speecht_amd.language_model import LanguageModel
  lm = LanguageModel.load(TINY) if with_lm else None
  logits, lens = HC.streams(29, 10 * beam + (3 if with_lm else 0))
  sets, which = _sets(29), [1, 2, 0]                                # two phrase sets and the empty one
  eng = _engine(dev, logits, lens)
  for k, n_best in enumerate((min(3, beam), beam)):
    per_set = {j: _offline_lists(eng, n_best, beam, lm, 0, sets.tables(j)) for j in set(which)}
    want = [per_set[j][s] for s, j in enumerate(which)]
    h = ListHarness(dev, logits, lens, beam, n_best, lm, 0, sets, which)
    ids, lp = h.run(([3, 1, 7, 2], [10, 4], [2, 9, 1, 1, 5]) if k else [HC.T] * 3)
    _check_run(h, want, ids, lp)
    assert want[2] == _offline_lists(eng, n_best, beam, lm, 0)[2]   # set 0: the unbiased search's list
  assert want[0] != _offline_lists(eng, n_best, beam, lm, 0)[0]     # the bias is at work


# ---- 3. / 4. open streams; an arena that is too small ------------------------------------------------------------------------------

def test_open_streams_write_nothing(dev):
  logits, lens = SC.cases29(7)
  h = ListHarness(dev, logits, lens, 16, 16)
  for _ in range(3):
    h.step({0: 5, 1: 2, 2: 9})                                      # (the harness asserts used == 0 and the fill pattern)
    assert h.demand == 0 and h.records == {}
  assert h.reads == 3 and h.lists == {}


@pytest.mark.parametrize('beam,kind', [(16, 'free'), (100, '3')])
def test_an_arena_that_is_too_small_loses_whole_lists(dev, beam, kind):
  from speecht_amd import nbest
  logits, lens = _inputs(kind, beam)
  lm = _model(None, 3)[0] if kind == '3' else None
  big = ListHarness(dev, logits, lens, beam, beam, lm, 0)
  big.run([80] * 5)                                                 # all five streams finish in one step
  assert big.reads == 1 and len(big.records) == 5
  full, demand = big.raw_arena, big.demand
  sizes, at = {}, 0
  while at < demand:                                                # the records in their order of arrival
    sizes[int(full[at])] = int(full[at + 4])
    at += int(full[at + 4])
  order = list(sizes)
  # room for exactly the first two records of that run -- and, since the order of arrival may differ from run to run, for the two
  # largest, where whichever record comes first must fit
  for cap, least in ((sizes[order[0]] + sizes[order[1]], 0), (sum(sorted(sizes.values())[-2:]), 1)):
    small = ListHarness(dev, logits, lens, beam, beam, lm, 0, arena_words=cap)
    small.run([80] * 5)                                             # (the harness checks result, tail and the words behind the arena)
    assert small.demand == demand and demand > cap
    kept = sorted(s for _, s in small.records)
    assert least <= len(kept) < 5 and sum(sizes[s] for s in kept) <= cap
    if [int(small.raw_arena[0]), int(small.raw_arena[sizes[order[0]]])] == order[:2] and not least:
      assert kept == sorted(order[:2])                              # the same arrivals: exactly the two records that fit
    for s in kept:                                                  # whichever arrived first this time: whole, and the big run's
      assert small.lists[s] == big.lists[s]
    assert (small.raw_arena[sum(sizes[s] for s in kept):] == FILL).all()   # nothing of a record that did not fit
    lists, lost = nbest.read_arena(small.raw_arena, demand, {(0, s): [] for s in range(5)})
    assert lost == demand - sum(sizes[s] for s in kept) > 0
  zero = ListHarness(dev, logits, lens, beam, beam, lm, 0, arena_words=0)
  zero.run([80] * 5)
  assert zero.demand == demand and zero.records == {} and zero.hyp == big.hyp


# ---- 5. endpointed pieces ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('beam,with_lm', [(16, False), (100, True)])
def test_pieces_write_a_list_per_final_with_its_piece_index(dev, beam, with_lm):
  """One step whose pieces -- laid out as the endpoint kernel writes them: {first row, rows, limit, reset} -- close two utterances of
  stream 0 and leave a third open, while stream 1 runs beside it without an event.  Rows: tests/endpoint_cases.py's streams."""
  from speecht_amd import nbest
  from speecht_amd.language_model import LanguageModel
  from tests import endpoint_cases as EC
  lm = LanguageModel.load(TINY) if with_lm else None
  x = EC.stream_logits(5, 70, 29, 27, 2, 3, 40)
  other = EC.stream_logits(6, 30, 29, 27, 2, 3, 40)
  nA, nB, nC = 31, 22, 17
  logits = np.zeros((70, 2, 29), np.float32)
  logits[:, 0], logits[:30, 1] = x, other
  n_best = min(beam, 5)
  h = ListHarness(dev, logits, [70, 30], beam, n_best, lm, 0)
  first_step = 9
  h.step({0: first_step})                                          # an ordinary open step first: the first final has stable labels or not
  rows = np.array([(0, first_step + j) for j in range(70 - first_step)] + [(1, j) for j in range(30)], np.int32)
  buf = np.full((len(rows), 32), 9.0, np.float32)
  buf[:70 - first_step, :29], buf[70 - first_step:, :29] = x[first_step:], other
  P = 3
  pieces = np.zeros((P, 2, 4), np.int32)
  pieces[:, :, 2] = -1
  pieces[0, 0] = (0, nA - first_step, nA, 0)
  pieces[1, 0] = (nA - first_step, nB, nA + nB, 1)
  pieces[2, 0] = (nA - first_step + nB, nC, -1, 1)
  pieces[0, 1] = (70 - first_step, 30, -1, 1)
  d_buf, d_rows, d_pieces = (torch.from_numpy(a).to(dev) for a in (buf, rows, pieces))
  tail = torch.full((P * 2 * h.max_tail,), -77, dtype=torch.int32, device=dev)
  result = torch.full((P * 2 * 4,), -77, dtype=torch.int32, device=dev)
  state2, pool2, tail2, result2 = h.state.clone(), h.pool.clone(), tail.clone(), result.clone()   # (a reset piece reuses the pool's nodes)
  args = lambda st, pl, tl, rs: (_ptr(d_buf), 32, 29, _ptr(d_rows), _ptr(d_pieces), P, len(rows), 2, beam, 0, h.handle, *_f(WEIGHTS), _ptr(st),
                                 _ptr(pl), h.max_frames, _ptr(h.ws), h.ws_bytes, _ptr(tl), h.max_tail, _ptr(rs), None)
  held = list(h.hyp[0][:h.stable[0]])
  h.lib.call('st_ctc_beam_stream_step_pieces_nbest', *args(h.state, h.pool, tail, result), None, None, n_best, _ptr(h.arena), h.cap, _ptr(h.used))
  torch.cuda.synchronize()
  arena, used = h.arena.cpu().numpy(), int(h.used.item())
  h.lib.call('st_ctc_beam_stream_step_pieces', *args(state2, pool2, tail2, result2))  # the same step without lists, on the copies
  torch.cuda.synchronize()
  assert torch.equal(tail, tail2) and torch.equal(result, result2) and torch.equal(h.pool, pool2)
  stride = int(h.raw.st_ctc_beam_stream_state_bytes(beam, int(with_lm))) // 8
  headers = lambda st: st[:2 * stride].view(2, stride)[:, :4]       # (a search saves its dead entries as the LDS held them: the headers)
  assert torch.equal(headers(h.state), headers(state2))
  assert (arena[h.cap:] == FILL).all() and (arena[used:] == FILL).all() and h.pattern_intact()
  lists, lost = nbest.read_arena(arena[:h.cap], used, {(0, 0): held, (1, 0): []})
  assert lost == 0 and sorted(lists) == [(0, 0), (1, 0)]           # the piece index is the header's; the open pieces wrote nothing
  batch = np.zeros((max(nA, nB), 2, 29), np.float32)
  batch[:nA, 0], batch[:nB, 1] = x[:nA], x[nA:nA + nB]
  want = _offline_lists(_engine(dev, batch, [nA, nB]), n_best, beam, lm, 0)
  got = [[(hyp['ids'], np.float32(hyp['log_prob']).tobytes()) for hyp in lists[key]] for key in ((0, 0), (1, 0))]
  assert got == want and len(want[0]) > 1
  res = result.cpu().numpy().reshape(P, 2, 4)
  assert [(len(l[0][0]), np.frombuffer(l[0][1], np.int32)[0]) for l in got] == [(res[0, 0, 0], res[0, 0, 2]), (res[1, 0, 0], res[1, 0, 2])]


# ---- 6. - 8. the layers above ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def tiny(dev):
  from speecht_amd.engine import Wav2LetterEngine
  from tests import endpoint_cases as EC
  layers, params = EC.recognizer_model()
  eng = Wav2LetterEngine(layers, device=dev)
  eng.set_weights(params)
  return eng


def _second_model(tmp_path_factory):
  return _model(str(tmp_path_factory.getbasetemp()), 2)[0]


def _list_key(hyps):
  return None if hyps is None else [(h['ids'], np.float64(h['log_prob']).tobytes(), sorted((k, repr(v)) for k, v in h.items())) for h in hyps]


def test_recognizer_finals_carry_the_offline_lists_and_their_rescoring(dev, tiny, tmp_path_factory):
  """(The endpointed model of tests/endpoint_cases.py: the small fixture of test_gpu_stream_beam.py never falls silent.)"""
  from speecht_amd import nbest
  from speecht_amd.language_model import LanguageModel
  from speecht_amd.streaming import FinalWords, StreamBeam, StreamingRecognizer
  from tests import endpoint_cases as EC
  from tests.test_gpu_endpoint import _endpointing, _key, _offline_batch, _stream
  from tests.test_gpu_stream_words import _check_final_words
  lm = LanguageModel.load(TINY)
  xa = EC.recognizer_features('a')
  make = lambda **kw: StreamingRecognizer(tiny, 1, max_chunk_frames=64, beam=StreamBeam(beam_width=16, lm=lm, nbest=4, **kw),
                                          endpoint=_endpointing(), words=FinalWords(timestamps=True))
  rec = make()
  finals, logits, _, _ = _stream(rec, rec.open(), xa, 50)
  rec2 = make()
  finals2, logits2, _, _ = _stream(rec2, rec2.open(), xa, 37)
  assert logits.tobytes() == logits2.tobytes() and len(finals) >= 2
  assert [_key(u) for u in finals] == [_key(u) for u in finals2]
  assert [_list_key(u.nbest) for u in finals] == [_list_key(u.nbest) for u in finals2] and all(u.nbest for u in finals)
  eng, _ = _offline_batch(dev, [logits[u.start_frame:u.end_frame] for u in finals], 29)
  first = nbest.components(eng, lm, eng.lm_beam_search_decode_nbest(lm, 4, 16), (0.8, 0.0, 2.3))
  assert [_list_key(u.nbest) for u in finals] == [_list_key(l) for l in first]
  assert all(u.ids == u.nbest[0]['ids'] and np.float32(u.logp).tobytes() == np.float32(u.nbest[0]['log_prob']).tobytes() for u in finals)
  assert max(len(u.nbest) for u in finals) > 1
  # the same finals without lists: the first pass's bits, words included
  plain = StreamingRecognizer(tiny, 1, max_chunk_frames=64, beam=StreamBeam(beam_width=16, lm=lm), endpoint=_endpointing(),
                              words=FinalWords(timestamps=True))
  base, _, _, _ = _stream(plain, plain.open(), xa, 50)
  assert [_key(u) for u in base] == [_key(u) for u in finals] and all(u.nbest is None for u in base)
  assert [None if u.spans is None else u.spans.tobytes() for u in base] == [None if u.spans is None else u.spans.tobytes() for u in finals]
  # rescoring under a second model, weighted so heavily that it decides
  lm2 = _second_model(tmp_path_factory)
  options = dict(language_model=lm2, lm_weight=6.0)
  again = make(rescore=options)
  refinals, relogits, _, _ = _stream(again, again.open(), xa, 50)
  assert relogits.tobytes() == logits.tobytes()
  want = nbest.rescored(first, eng, lm2, 6.0, 0.0, 2.3)
  assert [_list_key(u.nbest) for u in refinals] == [_list_key(l) for l in want]
  assert all(u.ids == u.nbest[0]['ids'] and u.logp == u.nbest[0]['log_prob'] for u in refinals)
  assert any(u.ids != v.ids for u, v in zip(refinals, finals))      # a final changed its first hypothesis
  assert [(u.start_frame, u.end_frame, u.greedy_ids) for u in refinals] == [(u.start_frame, u.end_frame, u.greedy_ids) for u in finals]
  assert _check_final_words_spans(refinals, logits, dev) >= 1


def _check_final_words_spans(finals, logits, dev):
  """The spans belong to the ids that are reported: ``engine.align``'s on the utterance's rows."""
  from tests.test_gpu_endpoint import _offline_batch
  some = 0
  for u in finals:
    if len(u.ids) == 0 or u.spans is None:
      continue
    eng, _ = _offline_batch(dev, [logits[u.start_frame:u.end_frame]], 29)
    spans = eng.align([u.ids])[0]
    assert np.array_equal(np.asarray(spans[0]), u.spans)
    some += 1
  return some


def test_lists_at_finish_and_nbest_none_is_untouched(dev, tiny):
  from speecht_amd import nbest
  from speecht_amd._lib import launch_trace
  from speecht_amd.streaming import StreamBeam, StreamingRecognizer
  from tests import endpoint_cases as EC
  x = EC.recognizer_features('b')[:300]

  def run(beam, chunk=50):
    rec = StreamingRecognizer(tiny, 2, max_chunk_frames=64, beam=beam)
    slot, seen, rows, counts = rec.open(), [], [], []
    with launch_trace() as tr:
      for at in range(0, len(x), chunk):
        r = rec.step({slot: x[at:at + chunk]}, return_logits=True)
        rows.append(r.logits[slot])
        counts.append(rec.launches)
        seen.append((r.hyp[slot], r.stable[slot], np.float32(r.logp[slot]).tobytes(), r.nbest.get(slot), r.nbest_lost.get(slot)))
      r = rec.finish(slot, return_logits=True)
      rows.append(r.logits[slot])
      counts.append(rec.launches)
    return rec, r, seen, np.concatenate(rows), counts, tr.lines

  plain, r0, seen0, logits, counts0, lines0 = run(StreamBeam(beam_width=16, max_seconds=8.0))
  assert not any('nbest' in l for l in lines0) and sum(l.startswith('ctc_beam_stream_read<') for l in lines0) == len(counts0)
  assert not hasattr(plain, 'nbest_arena') and not hasattr(plain._beam, 'arena') and r0.nbest == {} and r0.nbest_lost == {}
  greedy = StreamingRecognizer(tiny, 2, max_chunk_frames=64)
  g = greedy.open()
  for at in range(0, 200, 50):
    greedy.step({g: x[at:at + 50]})
  assert counts0[3] == greedy.launches + 3                         # (a step with rows) what tests/test_gpu_stream_beam.py pins
  assert plain.dec_out.numel() == 2 * plain.max_new + 4 + 2 * (4 + 256)
  # with lists: one enqueue more per pass (the counter's reset), the same hypotheses, and the list at finish
  listed, r1, seen1, logits1, counts1, lines1 = run(StreamBeam(beam_width=16, max_seconds=8.0, nbest=5))
  assert logits1.tobytes() == logits.tobytes() and counts1 == [c + 1 for c in counts0]
  assert [s[:3] for s in seen1] == [s[:3] for s in seen0] and all(s[3] is None and s[4] == 0 for s in seen1)
  assert sum(l.startswith('ctc_beam_stream_read_nbest<') for l in lines1) == len(counts1) and listed.dec_out.numel() == plain.dec_out.numel() + 1
  slot = 0
  assert (r1.hyp[slot], np.float32(r1.logp[slot]).tobytes()) == (r0.hyp[slot], np.float32(r0.logp[slot]).tobytes())
  eng = _engine(dev, logits[:, None, :], [300 // 2])
  want = nbest.components(eng, None, eng.beam_search_decode_nbest(5, 16))
  assert _list_key(r1.nbest[slot]) == _list_key(want[0]) and r1.nbest_lost[slot] == 0 and len(want[0]) == 5
  # an arena without room: the list is lost and counted, the hypothesis stays
  _, r2, _, _, _, _ = run(StreamBeam(beam_width=16, max_seconds=8.0, nbest=5, nbest_words=7))
  assert r2.nbest[slot] is None and r2.nbest_lost[slot] == 1 and r2.hyp[slot] == r0.hyp[slot]


def test_cli_stream_prints_the_reranked_lists(dev, golden_dir, tmp_path, tmp_path_factory, capsys, monkeypatch):
  from speecht_amd import vocabulary
  from speecht_amd.speech_input import SingleInputLoader
  from speecht_amd.speech_model import Session, Wav2LetterModel
  loader = importlib.machinery.SourceFileLoader('speecht_cli_stream_nbest_gpu', os.path.join(ROOT, 'speecht-cli'))
  spec = importlib.util.spec_from_loader(loader.name, loader)
  cli = importlib.util.module_from_spec(spec)
  loader.exec_module(cli)
  flac = os.path.join(golden_dir, '1089-134686-0037.flac')
  model = Wav2LetterModel(SingleInputLoader(128), 128, 29)         # a checkpoint written the way test_gpu_stream.py does
  model.add_training_ops()
  model.add_decoding_ops()
  model.finalize(str(tmp_path / 'log'), 'r', 'record')
  model.init_seed = 1234
  train = tmp_path / 'train'
  (train / 'run').mkdir(parents=True)
  with Session(dev) as sess:
    model.init_session(sess)
    model.saver.save(sess, str(train / 'run' / 'speechT'), global_step=model.global_step)
  _second_model(tmp_path_factory)
  second = os.path.join(str(tmp_path_factory.getbasetemp()), 'r2.arpa')
  cwd = tmp_path / 'cwd'
  cwd.mkdir()
  monkeypatch.chdir(cwd)
  base = ['stream', '--train-dir', str(train), '--run-name', 'run', '--device', dev, '--beam-width', '16', '--language-model', TINY]
  capsys.readouterr()
  code = cli.main(base + ['--endpoint', '--endpoint-silence', '0.1', '--endpoint-lead', '0.3', '--max-utterance', '1.5', '--nbest', '3',
                          '--rescore-language-model', second, '--rescore-lm-weight', '2.0', flac])
  lines = capsys.readouterr().out.splitlines()
  assert code == 0
  utts, ranked, k = [], [], 0
  while k < len(lines) - 1:
    f = lines[k].split('\t')
    if f[0] == 'utt':
      hyps = []
      while k + 1 < len(lines) - 1 and lines[k + 1].split('\t')[0] == flac:
        k += 1
        g = lines[k].split('\t')
        assert len(g) == 4 and int(g[1]) == len(hyps) + 1
        hyps.append(g)
      assert 1 <= len(hyps) <= 3 and hyps[0][3] == f[4]            # the final's transcript is the re-ranked first hypothesis's
      assert all(float(a[2]) >= float(b[2]) for a, b in zip(hyps, hyps[1:]))
      utts.append(f[4])
      ranked.append(hyps)
    k += 1
  assert len(utts) >= 1 and any(len(h) > 1 for h in ranked)
  assert lines[-1] == '{}\t{}'.format(flac, ' '.join(utts))         # the closing transcript joins the re-ranked finals
  # without --endpoint the list follows the closing line
  code = cli.main(base + ['--nbest', '3', flac])
  lines = capsys.readouterr().out.splitlines()
  assert code == 0
  at = max(k for k, l in enumerate(lines) if l.startswith(flac + '\t') and len(l.split('\t')) == 2)
  listed = [l.split('\t') for l in lines[at + 1:]]
  assert 1 <= len(listed) <= 3 and [g[:2] for g in listed] == [[flac, str(i + 1)] for i in range(len(listed))]
  assert lines[at] == '{}\t{}'.format(flac, listed[0][3])
  assert sorted(os.listdir(str(cwd))) == []


def test_recognizer_lists_carry_each_streams_own_hotword_set(dev):
  """Three streams of one recogniser, each opened with another phrase set (two sets and the empty set 0), finished together: every
  list is `nbest.components` of the offline biased search with that stream's set -- `bias` and an `acoustic` without it -- and set 0
  gives the unbiased list without a `bias`."""
  from speecht_amd import nbest
  from speecht_amd.engine import Wav2LetterEngine
  from speecht_amd.streaming import StreamBeam, StreamingRecognizer
  from tests import workloads as WL
  from tests.test_gpu_stream_hotwords import SMALL, _network_phrases
  params = WL.xavier_params(SMALL, seed=7)
  params[-1] = (params[-1][0] * 12.0, params[-1][1] * 4.0)        # (the small fixture of tests/test_gpu_stream_beam.py)
  small = Wav2LetterEngine(SMALL, device=dev)
  small.set_weights(params)
  x = WL.synthetic_features(151, 151, 16).astype(np.float32)
  sets, _ = _network_phrases(small, x)
  rec = StreamingRecognizer(small, 3, max_chunk_frames=64, beam=StreamBeam(beam_width=16, max_seconds=4.0, hotwords=sets, nbest=4))
  slots = {k: rec.open(hotwords=k) for k in (1, 2, 0)}
  rows = []
  for at in range(0, len(x), 50):
    r = rec.step({s: x[at:at + 50] for s in slots.values()}, return_logits=True)
    rows.append(r.logits[slots[1]])
    assert all(r.nbest[s] is None for s in slots.values())
  r = rec.finish_many(list(slots.values()), return_logits=True)
  logits = np.concatenate(rows + [r.logits[slots[1]]])
  eng = _engine(dev, logits[:, None, :], [151 // 2])
  for k, s in slots.items():
    hw = sets.tables(k) if k else None
    want = nbest.components(eng, None, eng.beam_search_decode_nbest(4, 16, hotwords=sets.tables(k)), hotwords=hw)[0]
    assert _list_key(r.nbest[s]) == _list_key(want) and r.nbest_lost[s] == 0 and len(want) == 4, k
    assert r.hyp[s] == want[0]['ids'] and np.float32(r.logp[s]).tobytes() == np.float32(want[0]['log_prob']).tobytes()
    if k:
      assert all(h['bias'] == hw.score(h['ids'])[1] and h['acoustic'] == h['log_prob'] - h['bias'] for h in r.nbest[s])
    else:
      assert all('bias' not in h and h['acoustic'] == h['log_prob'] for h in r.nbest[s])
      assert _list_key(r.nbest[s]) == _list_key(nbest.components(eng, None, eng.beam_search_decode_nbest(4, 16))[0])
  assert any(h['bias'] > 0 for k in (1, 2) for h in r.nbest[slots[k]])
  assert _list_key(r.nbest[slots[1]]) != _list_key(r.nbest[slots[0]])


def test_a_failed_stream_does_not_cost_the_others_their_lists(dev, tiny):
  """Two streams finish in one pass; one has more labels open than ``max_tail`` takes, so the host gives up on it -- the device wrote
  its record all the same.  The pass ends in that stream's `StreamError`, as without lists, with the other stream's list attached."""
  from speecht_amd.streaming import StreamBeam, StreamError, StreamingRecognizer
  from tests import endpoint_cases as EC
  x = EC.recognizer_features('b')[:300]
  quiet = np.zeros((120, 16), np.float32)

  def run(max_tail):
    rec = StreamingRecognizer(tiny, 2, max_chunk_frames=64,
                              beam=StreamBeam(beam_width=16, max_seconds=8.0, nbest=3, max_tail=max_tail, nbest_words=8192))
    a, b = rec.open(), rec.open()
    for at in range(0, len(x), 60):
      rec.step({a: x[at:at + 60], b: quiet[at:at + 60]}, fetch=False)   # (no read-out before the end: nothing is stable yet)
    return rec, a, b

  rec, a, b = run(256)
  whole = rec.finish_many([a, b])
  if len(whole.hyp[b]) > len(whole.hyp[a]):                        # (whichever is longer plays the failing part)
    a, b = b, a
  short, long_ = len(whole.hyp[b]), len(whole.hyp[a])
  assert 0 < short < long_                                         # a tail limit between the two: stream a's read-out gives up, b's does not
  good, bad = b, a
  rec, a, b = run(short)
  a, b = bad, good
  with pytest.raises(StreamError, match='stream {}: the beam search gave up'.format(a)) as failure:
    rec.finish_many([a, b])
  r = failure.value.result
  assert rec._beam.failed[a] and not rec._beam.failed[b], (rec._beam.failed, r.hyp, r.nbest_lost)
  assert r.nbest[a] is None and r.nbest_lost[b] == 0 and r.nbest[b] is not None, (r.nbest, r.nbest_lost)
  assert _list_key(r.nbest[b]) == _list_key(whole.nbest[b]) and r.hyp[b] == whole.hyp[b] and 1 <= len(r.nbest[b]) <= 3
