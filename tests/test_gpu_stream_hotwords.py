"""Hotword biasing of the streaming beam searches, a phrase set per stream (st_ctc_beam_stream_step_bias / _read_bias /
_step_pieces_bias, StreamBeam(hotwords=...), `speecht-cli stream --hotword`): however a stream's rows are cut, the finishing read
returns the ids, the length and -- bit for bit -- the log-probability of the biased whole-utterance searches on the same rows with
the stream's own set; streams of one launch have sets of their own, and the empty set is the unbiased search; partial results equal
the float64 specification (tests/stream_hotword_oracle.py) on inputs tests/test_stream_hotwords_cpu.py has vetted; an endpoint
forfeits an open match and the next utterance starts at the set's root; records of the two kinds do not mix; the layers above."""
import ctypes
import importlib.machinery
import importlib.util
import os

import numpy as np
import pytest

from tests import lm_oracle as L
from tests import stream_hotword_cases as HC
from tests import workloads as WL
from tests.test_lm_oracle_cpu import word_logits

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests.test_gpu_lm_beam import TINY, _engine  # noqa: E402  (after the importorskip, as that module does its own)

PATTERN = 0x5A5A5A5A5A5A5A5A
WEIGHTS = (0.8, 0.0, 2.3, -1000.0)
INERT = (0.0, 0.0, 0.0, -1000.0)                                  # a model that decides nothing: the LM kernels on LM-free scores
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


@pytest.fixture(scope='module')
def tiny_lm():
  from speecht_amd.language_model import LanguageModel
  return LanguageModel.load(TINY)


def _ptr(t):
  return ctypes.c_void_p(t.data_ptr())


def _f(values):
  return [ctypes.c_float(v) for v in values]


def _sets(C):
  from speecht_amd.hotwords import Hotwords, HotwordSets
  return HotwordSets([Hotwords([list(p) for p in phrases], w) for phrases, w in HC.phrase_sets(C)])


class Harness:
  """S streams through the C ABI with the host's part of the contract (tests/test_gpu_stream_beam.py::Harness): the labels below a
  stream's stable length are kept from earlier reads, a read appends the reported tail.  ``sets`` (a HotwordSets) and ``which``
  (the set of every stream) select the biased entry points; sets=None the unbiased ones.  State and pool start as a pattern (the
  first step resets); the pool lies inside a larger tensor whose tail holds the pattern; the logits' columns from C on hold values
  the kernels must not look at."""

  def __init__(self, dev, logits, lens, beam, lm=None, transform=0, sets=None, which=None, max_frames=HC.POOL, max_tail=96,
               weights=WEIGHTS):
    from speecht_amd import _lib
    self.lib, self.raw = _lib, _lib.load()
    self.dev, self.logits, self.lens = dev, logits, [int(n) for n in lens]
    self.T, self.S, self.C = logits.shape
    self.beam, self.lm, self.transform, self.max_frames, self.max_tail = beam, lm, transform, max_frames, max_tail
    self.weights = weights
    self.handle = lm.device_handle(dev) if lm is not None else None
    plain = int(self.raw.st_ctc_beam_stream_state_bytes(beam, int(lm is not None)))
    biased = int(self.raw.st_ctc_beam_stream_bias_state_bytes(beam, int(lm is not None)))
    up = lambda n: -(-n // 64) * 64
    assert biased == up(32 + (128 if beam > 64 else 64) * ((212 if lm is not None else 40) + 8)) and plain <= biased < plain + 8 * 128 + 64
    self.sets = sets
    self.state_bytes = biased                                    # (room for either kind: test 5 runs both on one buffer, S = 1)
    self.pool_bytes = int(self.raw.st_ctc_beam_stream_pool_bytes(max_frames, beam))
    self.state = torch.full((self.S * self.state_bytes // 8,), PATTERN, dtype=torch.int64, device=dev)
    self.pool = torch.full((self.S * self.pool_bytes // 8 + 64,), PATTERN, dtype=torch.int64, device=dev)
    self.ws_bytes = int(self.raw.st_ctc_beam_stream_ws(self.S * (self.T + 4)))
    self.ws = torch.empty(self.ws_bytes // 4, dtype=torch.float32, device=dev)
    self.tail = torch.zeros(self.S * max_tail, dtype=torch.int32, device=dev)
    self.result = torch.zeros(self.S * 4, dtype=torch.int32, device=dev)
    self.bias = ()
    if sets is not None:
      self.tables = sets.device_tables(dev)
      self.struct = _lib.BiasTables(*[t.data_ptr() for t in self.tables], sets.n_states)
      self.roots = torch.tensor([sets.root(k) for k in which], dtype=torch.int32, device=dev)
      self.bias = (ctypes.byref(self.struct), _ptr(self.roots))
    self.fed, self.started = [0] * self.S, [False] * self.S
    self.hyp, self.stable, self.logp, self.status = [[] for _ in range(self.S)], [0] * self.S, [None] * self.S, [0] * self.S

  def step(self, takes, finishing=(), read=True, extra=0, biased=None, reset=None):
    """``takes``: {stream: rows}; a finishing stream gets its limit and ``extra`` rows past it (which must not be decoded)."""
    rows, table, chunks = [], np.zeros((self.S, 4), np.int32), []
    table[:, 2] = -1
    for s in sorted(set(takes) | set(finishing)):
      n = takes.get(s, 0)
      if s in finishing:
        n += min(extra, self.T - self.fed[s] - n)
      fresh = (0 if self.started[s] else 1) if reset is None else int(reset)
      if fresh:
        self.hyp[s], self.stable[s] = [], 0                        # a reset search reports from its first label again
      table[s] = (len(rows), n, self.lens[s] if s in finishing else -1, fresh)
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
    biased = bool(self.bias) if biased is None else biased
    self.lib.call('st_ctc_beam_stream_step' + ('_bias' if biased else ''), _ptr(d_buf), 32, self.C, _ptr(d_rows), _ptr(d_table), n_rows,
                  self.S, self.beam, self.transform, self.handle, *_f(self.weights), _ptr(self.state), _ptr(self.pool), self.max_frames,
                  _ptr(self.ws), self.ws_bytes, None, *(self.bias if biased else ()))
    if read:
      self.read(d_table, biased)
    return d_table

  def read(self, d_table, biased=None):
    biased = bool(self.bias) if biased is None else biased
    self.lib.call('st_ctc_beam_stream_read' + ('_bias' if biased else ''), _ptr(d_table), self.S, self.beam, self.handle, *_f(self.weights),
                  _ptr(self.state), _ptr(self.pool), self.max_frames, _ptr(self.tail), self.max_tail, _ptr(self.result), None,
                  *(self.bias if biased else ()))
    torch.cuda.synchronize()
    table = d_table.cpu().numpy()
    res, tail = self.result.cpu().numpy().reshape(self.S, 4), self.tail.cpu().numpy().reshape(self.S, self.max_tail)
    for s in range(self.S):
      if table[s, 1] > 0 or table[s, 2] >= 0 or table[s, 3]:
        length, old = int(res[s, 0]), self.stable[s]
        self.status[s] = int(res[s, 3])
        self.logp[s] = res[s, 2:3].view(np.float32)[0]
        if self.status[s] & 2:
          continue                                                # no state: nothing was reported
        assert 0 <= length - old <= self.max_tail, (s, length, old)
        self.hyp[s] = self.hyp[s][:old] + tail[s, :length - old].tolist()
        self.stable[s] = int(res[s, 1])
        assert self.stable[s] >= old

  def run(self, cuts, read_every_step=True, on_step=None):
    """Stream s takes cuts[s] rows per step (a list: its entries in turn, round and round) until its length is fed; the step that
    feeds its last rows finishes it."""
    live, k = set(range(self.S)), 0
    while live:
      takes, finishing = {}, set()
      for s in sorted(live):
        cut = cuts[s][k % len(cuts[s])] if isinstance(cuts[s], (list, tuple)) else cuts[s]
        n = min(cut, self.lens[s] - self.fed[s])
        takes[s] = n
        if self.fed[s] + n >= self.lens[s]:
          finishing.add(s)
      self.step(takes, finishing, read=read_every_step or bool(finishing), extra=3)
      if on_step:
        on_step(k, takes, finishing)
      live -= finishing
      k += 1
    return [list(h) for h in self.hyp], np.asarray(self.logp, np.float32)

  def pattern_intact(self):
    return bool((self.pool[self.S * self.pool_bytes // 8:] == PATTERN).all())


def _offline(eng, beam, lm, transform, hw, weights=WEIGHTS):
  """The biased whole-utterance search, n_best = 1 (existing entry points) -> (ids per utterance, log_prob float32 per utterance);
  hw None: the unbiased one."""
  name = 'log10_softmax' if transform else None
  if lm is None:
    lists = eng.beam_search_decode_nbest(1, beam, name, hotwords=hw)
  else:
    lists = eng.lm_beam_search_decode_nbest(lm, 1, beam, name, *weights, hotwords=hw)
  return [l[0][0] for l in lists], np.asarray([l[0][1] for l in lists], np.float32)


def _offline_per_stream(dev, logits, lens, beam, lm, transform, sets, which, weights=WEIGHTS):
  """Stream s's reference: the offline biased search on its rows with its own set's tables alone."""
  eng = _engine(dev, logits, lens)
  runs = {k: _offline(eng, beam, lm, transform, sets.tables(k), weights) for k in sorted(set(which))}
  return [runs[k][0][s] for s, k in enumerate(which)], np.asarray([runs[k][1][s] for s, k in enumerate(which)], np.float32)


# ---- 1. every cut returns the offline biased search -----------------------------------------------------------------------------

# candidates per lane of the instantiation a (beam, classes) pair launches: 4 / 8 / 16 / 32 at 64 entries, 64 = the wide form
DISPATCH = {(1, 29): 4, (16, 29): 8, (32, 29): 16, (64, 29): 32, (100, 29): 64, (128, 29): 64,
            (1, 5): 4, (16, 5): 4, (32, 5): 4, (64, 5): 8, (100, 5): 64, (128, 5): 64}
CUTS = ([1, 1, 1], [HC.T, HC.T, HC.T], [[3, 1, 7, 2], [10, 4], [2, 9, 1, 1, 5]])


@pytest.mark.parametrize('transform', [0, 1])
@pytest.mark.parametrize('kind', ['free', 'free5', 'lm'])
@pytest.mark.parametrize('beam', [1, 16, 32, 64, 100, 128])
def test_every_cut_returns_the_offline_biased_search_bit_for_bit(dev, tiny_lm, beam, kind, transform):
  from speecht_amd._lib import launch_trace
  C = 5 if kind == 'free5' else 29
  logits, lens = HC.streams(C, 10 * beam + transform + (3 if kind == 'lm' else 0))
  lm = tiny_lm if kind == 'lm' else None
  sets = _sets(C)
  ref_ids, ref_lp = _offline_per_stream(dev, logits, lens, beam, lm, transform, sets, HC.STREAM_SETS)
  seen = [False, False, False]
  for cuts in CUTS:
    h = Harness(dev, logits, lens, beam, lm, transform, sets, HC.STREAM_SETS)
    partial = []
    with launch_trace() as tr:
      ids, lp = h.run(cuts, on_step=lambda k, takes, finishing: partial.extend((s, list(h.hyp[s])) for s in takes))
    want = ('ctc_beam_stream_lm_bias<' if lm is not None else 'ctc_beam_stream_bias<') + ('wide' if beam > 64 else 'wave')
    searches = [l for l in tr.lines if l.startswith('ctc_beam_stream_') and '_read<' not in l]
    assert searches and all(l.startswith(want) and 'states={}'.format(sets.n_states) in l and l.endswith(' cpl={}'.format(DISPATCH[beam, C]))
                            for l in searches), tr.lines[:4]
    assert any(l.startswith('ctc_beam_stream_read<') and ', bias>' in l for l in tr.lines)
    assert ids == ref_ids, (cuts, ids, ref_ids)
    assert lp.tobytes() == ref_lp.tobytes(), (cuts, lp, ref_lp)
    assert h.status == [0] * len(lens) and h.pattern_intact()
    for s, hyp in partial:                                         # in what the streams reported, matches open, fail and complete
      seen = [a or b for a, b in zip(seen, HC.what_happened(sets.tables(HC.STREAM_SETS[s]).phrases, hyp))]
  assert seen[0] and seen[2], seen
  if C == 29:                                                      # (the five-class phrases overlap so much that another phrase nearly always
    assert seen[1], seen                                           # catches a broken match: credit is seldom given back there)
  unbiased = _offline(_engine(dev, logits, lens), beam, lm, transform, None)
  assert unbiased[0] != ref_ids or unbiased[1].tobytes() != ref_lp.tobytes()       # the bias is at work


def test_the_beams_cover_every_dispatch():
  """With and without a model (29 classes), test 1 launches all five instantiations: 4, 8, 16, 32 candidates per lane and wide."""
  assert {DISPATCH[b, 29] for b in (1, 16, 32, 64, 100, 128)} == {4, 8, 16, 32, 64}
  for (beam, C), cpl in DISPATCH.items():
    per_lane = -(-beam * C // 64)
    assert cpl == (64 if beam > 64 else next(c for c in (4, 8, 16, 32) if per_lane <= c))


# ---- 2. a set per stream ------------------------------------------------------------------------------------------------------

def _near_call():
  """Logits that spell 'the kat' with 'c' and 'b' half a nat behind 'k' on the frames of the k (tests/test_gpu_hotwords.py::_near_call),
  the same rows for three streams."""
  rng = np.random.default_rng(7)
  x = word_logits('the kat', rng, noise=0.3)
  k = L.LETTERS.index('k')
  for t in range(len(x)):
    if x[t].argmax() == k:
      x[t, L.LETTERS.index('c')] = x[t, L.LETTERS.index('b')] = x[t, k] - 0.5
  return np.repeat(x[:, None, :], 3, axis=1).astype(np.float32), [len(x)] * 3


@pytest.mark.parametrize('with_lm', [False, True])
@pytest.mark.parametrize('beam', [16, 128])
def test_streams_of_one_launch_have_sets_of_their_own(dev, tiny_lm, beam, with_lm):
  from speecht_amd.hotwords import Hotwords, HotwordSets
  logits, lens = _near_call()
  lm = tiny_lm if with_lm else None
  sets = HotwordSets([Hotwords(['the cat'], 0.3), Hotwords(['the bat', 'zebra'], 0.4)])
  which = [0, 1, 2]
  weights = INERT if with_lm else WEIGHTS                          # (as test_hotwords_decide_a_near_call: the model must not decide)
  ref_ids, ref_lp = _offline_per_stream(dev, logits, lens, beam, lm, 0, sets, which, weights)
  plain_ids, plain_lp = _offline(_engine(dev, logits, lens), beam, lm, 0, None, weights)
  biased = Harness(dev, logits, lens, beam, lm, 0, sets, which, weights=weights)
  ids, lp = biased.run([[4, 1, 6], [4, 1, 6], [4, 1, 6]])
  unbiased = Harness(dev, logits, lens, beam, lm, 0, weights=weights)
  ids0, lp0 = unbiased.run([[4, 1, 6], [4, 1, 6], [4, 1, 6]])
  assert [L.ids_to_text(i) for i in ids] == ['the kat', 'the cat', 'the bat']
  # stream 0, on the empty set, is the unbiased stream search -- and the unbiased whole-utterance search -- bits included
  assert ids[0] == ids0[0] == plain_ids[0] and lp[:1].tobytes() == lp0[:1].tobytes() == plain_lp[:1].tobytes()
  # streams 1 and 2 are their own offline biased searches
  assert ids == ref_ids and lp.tobytes() == ref_lp.tobytes()


# ---- 3. partial results ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', [c[0] for c in HC.EXACT])
def test_partials_equal_the_specification(dev, tiny_lm, name):
  logits, lens, beam, with_lm, transform = HC.exact_inputs(name)
  spec = HC.traces(name)
  h = Harness(dev, logits, lens, beam, tiny_lm if with_lm else None, 1 if transform else 0, _sets(logits.shape[2]), HC.STREAM_SETS)
  checked = [0]

  def check(k, takes, finishing):
    for s in takes:
      if s in finishing:
        continue                                                  # (the finishing read reports the whole-utterance result)
      n = h.fed[s]
      assert h.hyp[s] == spec[s]['hyp'][n], (name, s, n)
      assert h.stable[s] == spec[s]['stable'][n], (name, s, n)
      np.testing.assert_allclose(h.logp[s], spec[s]['logp'][n], rtol=1e-4, atol=1e-4)
      checked[0] += 1

  ids, lp = h.run([[7, 1, 3], 2, [1, 10]], on_step=check)
  assert checked[0] > 30
  assert ids == [tr['final'][0] for tr in spec]
  np.testing.assert_allclose(lp, [tr['final'][1] for tr in spec], rtol=1e-4, atol=1e-4)
  # a read-out changes nothing for the later steps
  quiet = Harness(dev, logits, lens, beam, tiny_lm if with_lm else None, 1 if transform else 0, _sets(logits.shape[2]), HC.STREAM_SETS)
  ids2, lp2 = quiet.run([[7, 1, 3], 2, [1, 10]], read_every_step=False)
  assert ids2 == ids and lp2.tobytes() == lp.tobytes()


# ---- 4. endpointed pieces ------------------------------------------------------------------------------------------------------

def _pieces_call(h, buf, rows, pieces, n_rows, P):
  """st_ctc_beam_stream_step_pieces_bias on host tables -> (result [P][S][4], tail [P][S][max_tail])."""
  S, mt = h.S, h.max_tail
  d_buf, d_rows = torch.from_numpy(buf).to(h.dev), torch.from_numpy(rows).to(h.dev)
  d_pieces = torch.from_numpy(pieces).to(h.dev)
  tail = torch.full((P * S * mt,), -77, dtype=torch.int32, device=h.dev)
  result = torch.full((P * S * 4,), -77, dtype=torch.int32, device=h.dev)
  h.lib.call('st_ctc_beam_stream_step_pieces_bias', _ptr(d_buf), 32, h.C, _ptr(d_rows), _ptr(d_pieces), P, n_rows, S, h.beam, h.transform,
             h.handle, *_f(h.weights), _ptr(h.state), _ptr(h.pool), h.max_frames, _ptr(h.ws), h.ws_bytes, _ptr(tail), mt, _ptr(result), None,
             *h.bias)
  torch.cuda.synchronize()
  return result.cpu().numpy().reshape(P, S, 4), tail.cpu().numpy().reshape(P, S, mt)


@pytest.mark.parametrize('with_lm', [False, True])
@pytest.mark.parametrize('beam', [16, 128])
def test_an_endpoint_forfeits_the_open_match_and_the_next_utterance_starts_at_the_root(dev, tiny_lm, beam, with_lm):
  """Pieces as the endpoint kernel writes them ({first row, rows, limit, reset}; include/speecht_hip.h) close two utterances of stream
  0 -- 'the ca' | 't sat on' | ' the mat' still open -- so that the phrase 'cat' straddles the first endpoint; stream 1 runs beside it
  without an event, on another set."""
  from speecht_amd._lib import launch_trace
  from speecht_amd.hotwords import Hotwords, HotwordSets
  lm = tiny_lm if with_lm else None
  weights = INERT if with_lm else WEIGHTS                          # ('ca' and 't' are no words: the model must not rewrite the text)
  rng = np.random.default_rng(11)
  parts = [word_logits(t, rng, frames_per_char=2, gap=1, noise=0.3, peak=5.0).astype(np.float32) for t in ('the ca', 't sat on', ' the mat')]
  other = word_logits('on the mat', rng, frames_per_char=2, gap=1, noise=0.3, peak=5.0).astype(np.float32)
  nA, nB, nC = (len(p) for p in parts)
  x = np.concatenate(parts)
  sets = HotwordSets([Hotwords(['cat', 'sat on', 'zeb'], 1.0), Hotwords(['mat', 'the'], 0.6)])
  T = len(x)
  logits = np.zeros((T, 2, 29), np.float32)
  logits[:, 0], logits[:len(other), 1] = x, other
  runs = []
  for first_step in (0, nA - 4):                                   # all rows in one step; the first final's rows over two steps
    h = Harness(dev, logits, [T, len(other)], beam, lm, 0, sets, [1, 2], max_frames=max(nA, nB, nC, len(other)), weights=weights)
    finals, opened = [], None
    if first_step:
      h.step({0: first_step}, read=True)                           # an ordinary open step: the match 'c' is lent credit
      opened = (list(h.hyp[0]), float(h.logp[0]))
    n0 = T - first_step
    rows = np.array([(0, first_step + j) for j in range(n0)] + [(1, j) for j in range(len(other))], np.int32)
    buf = np.full((len(rows), 32), 9.0, np.float32)
    buf[:n0, :29], buf[n0:, :29] = x[first_step:], other
    P = 3
    pieces = np.zeros((P, 2, 4), np.int32)
    pieces[:, :, 2] = -1
    pieces[0, 0] = (0, nA - first_step, nA, 0 if first_step else 1)
    pieces[1, 0] = (nA - first_step, nB, nA + nB, 1)
    pieces[2, 0] = (nA - first_step + nB, nC, -1, 1)
    pieces[0, 1] = (n0, len(other), -1, 1)
    with launch_trace() as tr:
      result, tail = _pieces_call(h, buf, rows, pieces, len(rows), P)
    want = 'ctc_beam_stream_lm_bias<' if with_lm else 'ctc_beam_stream_bias<'
    assert sum(l.startswith(want) for l in tr.lines) == sum(l.startswith('ctc_beam_stream_read<') and ', bias>' in l for l in tr.lines) == P
    assert (result[1:, 1] == -77).all()                            # an unused slot: both kernels left at once
    hyp, stable = list(h.hyp[0]), h.stable[0]
    for p in range(P):
      if pieces[p, 0, 3]:
        hyp, stable = [], 0
      length = int(result[p, 0, 0])
      assert result[p, 0, 3] == 0 and 0 <= length - stable <= h.max_tail
      hyp = hyp[:stable] + tail[p, 0, :length - stable].tolist()
      stable = int(result[p, 0, 1])
      finals.append((list(hyp), int(result[p, 0, 2])))
    runs.append((finals, opened))
    assert h.pattern_intact()
  assert runs[0][0] == runs[1][0]                                  # the same finals, bit for bit, for both cuts
  (ids_a, lp_a), (ids_b, lp_b), (ids_c, lp_c) = runs[0][0]
  assert [L.ids_to_text(i) for i in (ids_a, ids_b, ids_c)] == ['the ca', 't sat on', ' the mat']
  # each final is the offline biased search on its utterance's rows alone
  batch = np.zeros((max(nA, nB), 2, 29), np.float32)
  batch[:nA, 0], batch[:nB, 1] = parts[0], parts[1]
  eng = _engine(dev, batch, [nA, nB])
  ref_ids, ref_lp = _offline(eng, beam, lm, 0, sets.tables(1), weights)
  assert [ids_a, ids_b] == ref_ids and [lp_a, lp_b] == ref_lp.view(np.int32).tolist()
  # the credit of 'ca' is forfeited at the final: no bias is left in A's score, though the open stream had been lent some
  hw = sets.tables(1)
  assert hw.score(ids_a) == (2.0, 0.0)
  # (in the score itself this shows as equality with the offline search above, whose split into acoustic part and bias
  # tests/test_gpu_hotwords.py checks; a comparison with the UNBIASED search's score would only hold up to what the two beams prune)
  open_hyp, open_lp = runs[1][1]                                   # the open stream four rows before the endpoint: 'the c', one character lent
  assert L.ids_to_text(open_hyp) == 'the c' and hw.score(open_hyp)[0] == 1.0
  # the state did not leak: B starts at the root, so its 't' completes nothing -- the joined text would have banked 'cat'
  assert hw.score(ids_a + ids_b)[1] == hw.score(ids_a)[1] + hw.score(ids_b)[1] + 3.0
  assert hw.score(ids_b) == (6.0, 6.0)                             # 'sat on', inside B, is banked
  # the open third utterance carries lent credit only if a match is open at its end: ' the mat' under set 1 has none
  assert hw.score(ids_c) == (0.0, 0.0)


# ---- 5. records of the two kinds do not mix; refused requests -------------------------------------------------------------------------

@pytest.mark.parametrize('with_lm', [False, True])
def test_records_of_the_two_kinds_do_not_mix(dev, tiny_lm, with_lm):
  lm = tiny_lm if with_lm else None
  logits, lens = HC.streams(29, 5)
  logits, lens = logits[:, :1], lens[:1]                           # one stream: its record lies at the buffer's start for both kinds
  sets = _sets(29)
  for first_biased in (False, True):
    h = Harness(dev, logits, lens, 16, lm, 0, sets, [1])
    h.step({0: 10}, biased=first_biased)
    assert h.status == [0] and len(h.hyp[0]) > 0
    before = h.state.clone()
    kept = (list(h.hyp[0]), h.stable[0])
    h.step({0: 10}, biased=not first_biased)                        # no reset: the other kind's record is nothing to continue
    assert torch.equal(h.state, before)
    assert h.status == [2] and h.logp[0] == -np.inf and (list(h.hyp[0]), h.stable[0]) == kept
    h.fed[0] -= 10
    h.step({0: 10}, biased=first_biased)                            # ... and its own kind goes on as if nothing had happened
    solo = Harness(dev, logits, lens, 16, lm, 0, sets, [1])
    solo.step({0: 10}, biased=first_biased)
    solo.step({0: 10}, biased=first_biased)
    assert h.status == [0] and h.hyp == solo.hyp and np.float32(h.logp[0]).tobytes() == np.float32(solo.logp[0]).tobytes()
    h.step({0: 5}, biased=not first_biased, reset=True)             # a reset makes the record the other kind's
    assert h.status == [0]


def test_validation_returns_an_error_without_a_launch(dev, tiny_lm):
  from speecht_amd import _lib
  from speecht_amd._lib import launch_trace
  lib = _lib.load()
  assert lib.st_ctc_beam_stream_bias_state_bytes(0, 0) == 0 and lib.st_ctc_beam_stream_bias_state_bytes(129, 1) == 0
  up = lambda n: -(-n // 64) * 64                                 # 8 B per entry on top of the unbiased record
  assert lib.st_ctc_beam_stream_bias_state_bytes(64, 1) == up(32 + 64 * 220) and lib.st_ctc_beam_stream_bias_state_bytes(65, 1) == up(32 + 128 * 220)
  assert lib.st_ctc_beam_stream_bias_state_bytes(16, 0) == up(32 + 64 * 48)
  assert lib.st_ctc_beam_stream_state_bytes(64, 1) == up(32 + 64 * 212) and lib.st_ctc_beam_stream_state_bytes(16, 0) == up(32 + 64 * 40)
  z = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device=dev)
  logits, rows, table = z(4 * 32, torch.float32), z(8), z(12)
  state, pool, ws, tail, result = z(32 + 128 * 220, torch.uint8), z(2 * 4096), z(4 * 32, torch.float32), z(3 * 64), z(12)
  nxt, gain, fin, roots = z(32), z(32, torch.float32), z(1, torch.float32), z(1)
  handle = tiny_lm.device_handle(dev)

  def tables(**spoil):
    fields = dict(next=nxt.data_ptr(), gain=gain.data_ptr(), fin=fin.data_ptr(), n_states=1)
    fields.update(spoil)
    return _lib.BiasTables(fields['next'], fields['gain'], fields['fin'], fields['n_states'])

  ok = dict(C=29, lm=handle, bias=tables(), roots=_ptr(roots))

  def step(**kw):
    a = dict(ok, **kw)
    return lib.st_ctc_beam_stream_step_bias(_ptr(logits), 32, a['C'], _ptr(rows), _ptr(table), 4, 1, 16, 0, a['lm'], *_f(WEIGHTS), _ptr(state),
                                            _ptr(pool), 16, _ptr(ws), 4 * 32 * 4, None, a['bias'] and ctypes.byref(a['bias']), a['roots'])

  def read(**kw):
    a = dict(ok, **kw)
    return lib.st_ctc_beam_stream_read_bias(_ptr(table), 1, 16, a['lm'], *_f(WEIGHTS), _ptr(state), _ptr(pool), 16, _ptr(tail), 64,
                                            _ptr(result), None, a['bias'] and ctypes.byref(a['bias']), a['roots'])

  def pieces(**kw):
    a = dict(ok, **kw)
    return lib.st_ctc_beam_stream_step_pieces_bias(_ptr(logits), 32, a['C'], _ptr(rows), _ptr(table), 3, 4, 1, 16, 0, a['lm'], *_f(WEIGHTS),
                                                   _ptr(state), _ptr(pool), 16, _ptr(ws), 4 * 32 * 4, _ptr(tail), 64, _ptr(result), None,
                                                   a['bias'] and ctypes.byref(a['bias']), a['roots'])

  with launch_trace() as tr:
    for fn in (step, read, pieces):
      for kw, text in ((dict(bias=None), 'null hotword tables'), (dict(bias=tables(next=None)), 'null hotword tables'),
                       (dict(bias=tables(gain=None)), 'null hotword tables'), (dict(bias=tables(fin=None)), 'null hotword tables'),
                       (dict(bias=tables(n_states=0)), 'states supported'), (dict(bias=tables(n_states=-3)), 'states supported'),
                       (dict(roots=None), 'null argument')):
        assert fn(**kw) != 0, (fn.__name__, kw)
        assert text in lib.st_last_error().decode(), (fn.__name__, kw, lib.st_last_error().decode())
    for fn in (step, pieces):                                      # with a model: the 28 labels and the blank, no more, no fewer
      for C in (28, 30, 32):
        assert fn(C=C) != 0 and 'classes must be' in lib.st_last_error().decode(), C
      assert fn(C=33, lm=None) != 0 and 'classes' in lib.st_last_error().decode()
  assert tr.lines == []
  torch.cuda.synchronize()


# ---- 6. the layers above ------------------------------------------------------------------------------------------------------

SMALL = WL.w2l_layers(16, width=24, fc=40)


@pytest.fixture(scope='module')
def small(dev):
  from speecht_amd.engine import Wav2LetterEngine
  params = WL.xavier_params(SMALL, seed=7)
  params[-1] = (params[-1][0] * 12.0, params[-1][1] * 4.0)        # (peakier posteriors: the hypotheses are not all empty)
  eng = Wav2LetterEngine(SMALL, device=dev)
  eng.set_weights(params)
  return eng


def _solo(rec, slot, x, chunk):
  """One stream: [(input frames, hyp, stable, logp bits)] after every step and after the finish, and the logits."""
  seen, rows = [], []
  for at in range(0, len(x), chunk):
    r = rec.step({slot: x[at:at + chunk]}, return_logits=True)
    rows.append(r.logits[slot])
    seen.append((min(at + chunk, len(x)), r.hyp[slot], r.stable[slot], np.float32(r.logp[slot]).tobytes()))
  r = rec.finish(slot, return_logits=True)
  rows.append(r.logits[slot])
  seen.append(('end', r.hyp[slot], r.stable[slot], np.float32(r.logp[slot]).tobytes()))
  return seen, np.concatenate(rows)


def _network_phrases(small, x):
  """Phrase sets taken from what this random network says, so that the bias has something to hold on to."""
  from speecht_amd.hotwords import Hotwords, HotwordSets
  from speecht_amd.streaming import StreamBeam, StreamingRecognizer
  rec = StreamingRecognizer(small, 1, max_chunk_frames=64, beam=StreamBeam(beam_width=16, max_seconds=4.0))
  seen, _ = _solo(rec, rec.open(), x, 50)
  text = seen[-1][1]
  assert len(text) >= 8
  one = [text[i:i + 3] for i in range(0, len(text) - 2, 4)][:6]
  two = [text[i:i + 2] for i in range(1, len(text) - 1, 5)][:5] + [[25, 4, 1]]
  return HotwordSets([Hotwords(one, 1.5), Hotwords(two, 0.8)]), seen


def test_whole_path_two_chunkings_and_a_reopened_slot(dev, small):
  from speecht_amd._lib import launch_trace
  from speecht_amd.streaming import StreamBeam, StreamError, StreamingRecognizer
  x = WL.synthetic_features(151, 151, 16).astype(np.float32)
  sets, plain = _network_phrases(small, x)
  make = lambda: StreamingRecognizer(small, 2, max_chunk_frames=64, beam=StreamBeam(beam_width=16, max_seconds=4.0, hotwords=sets))
  results = {}
  for k in (1, 2, 0):
    rec_a, rec_b = make(), make()
    with launch_trace() as tr:
      a, logits = _solo(rec_a, rec_a.open(hotwords=k), x, 50)
    assert any(l.startswith('ctc_beam_stream_bias<') for l in tr.lines) and not any(l.startswith('ctc_beam_stream<') for l in tr.lines)
    b, logits_b = _solo(rec_b, rec_b.open(hotwords=k), x, 25)
    assert np.array_equal(logits, logits_b)
    at = {key: v for key, *v in b}
    for key, *v in a:                                             # hyp, stable and logp where both runs have a step boundary
      assert at[key] == v, (k, key)
    stables = [s for _, _, s, _ in a]
    assert all(p <= q for p, q in zip(stables, stables[1:])) and a[-1][2] == len(a[-1][1])
    # the final hypothesis is the biased whole-utterance search on the stream's own logits, with the stream's own set
    eng = _engine(dev, logits[:, None, :], [151 // 2])
    ref_ids, ref_lp = eng.beam_search_decode_nbest(1, 16, hotwords=sets.tables(k))[0][0]
    assert a[-1][1] == ref_ids and a[-1][3] == np.float32(ref_lp).tobytes()
    results[k] = a
  assert [v[1:] for v in results[0]] == [v[1:] for v in plain]      # set 0: the unbiased recogniser's results, bits included
  assert results[1][-1][1:] != results[0][-1][1:] and results[2][-1][1:] != results[0][-1][1:]
  assert sets.tables(1).score(results[1][-1][1])[1] > 0
  # a reopened slot with another set index starts from that set's root; the default is set 0 with a HotwordSets
  rec = make()
  s = rec.open(hotwords=1)
  rec.step({s: x[:100]})
  rec.close(s)
  again = rec.open(hotwords=2)
  assert again == s
  got, _ = _solo(rec, again, x, 50)
  assert got == results[2]
  rec.close(again)
  got, _ = _solo(rec, rec.open(), x, 50)
  assert got == results[0]
  # one Hotwords: every stream uses it
  single = StreamingRecognizer(small, 1, max_chunk_frames=64, beam=StreamBeam(beam_width=16, max_seconds=4.0, hotwords=sets.tables(1)))
  got, _ = _solo(single, single.open(), x, 50)
  assert got == results[1]
  for bad in (3, -1, 1.5, True):
    with pytest.raises(StreamError, match='sets 0..2'):
      rec.open(hotwords=bad)
  with pytest.raises(StreamError, match='no beam search with hotwords'):
    StreamingRecognizer(small, 1, beam=StreamBeam(beam_width=16, max_seconds=4.0)).open(hotwords=0)
  with pytest.raises(StreamError, match='no beam search with hotwords'):
    StreamingRecognizer(small, 1).open(hotwords=1)


def test_endpointed_recognizer_finals_are_offline_biased_searches(dev):
  """StreamingRecognizer(beam=StreamBeam(hotwords=...), endpoint=...): the finals are identical between two chunkings and equal
  ``engine.beam_search_decode_nbest(..., hotwords=, n_best=1)`` on each utterance's rows alone."""
  from speecht_amd.engine import Wav2LetterEngine
  from speecht_amd.hotwords import Hotwords
  from speecht_amd.streaming import StreamBeam, StreamingRecognizer
  from tests import endpoint_cases as EC
  from tests.test_gpu_endpoint import _endpointing, _key, _offline_batch, _stream
  layers, params = EC.recognizer_model()
  tiny = Wav2LetterEngine(layers, device=dev)
  tiny.set_weights(params)
  xa = EC.recognizer_features('a')
  plain_rec = StreamingRecognizer(tiny, 1, max_chunk_frames=64, beam=StreamBeam(beam_width=16), endpoint=_endpointing())
  plain, _, _, _ = _stream(plain_rec, plain_rec.open(), xa, 50)
  texts = [u.ids for u in plain if len(u.ids) >= 3]
  assert texts
  hw = Hotwords([t[i:i + 3] for t in texts for i in range(0, len(t) - 2, 4)][:40] + ['zebra'], 1.2)
  make = lambda: StreamingRecognizer(tiny, 1, max_chunk_frames=64, beam=StreamBeam(beam_width=16, hotwords=hw), endpoint=_endpointing())
  rec = make()
  finals, logits, seen, _ = _stream(rec, rec.open(), xa, 50)
  rec2 = make()
  finals2, logits2, _, _ = _stream(rec2, rec2.open(), xa, 37)
  assert logits2.tobytes() == logits.tobytes() and [_key(u) for u in finals2] == [_key(u) for u in finals] and len(finals) >= 2
  assert [(u.start_frame, u.end_frame) for u in finals] == [(u.start_frame, u.end_frame) for u in plain]   # the endpoints are the greedy decoder's
  eng, _ = _offline_batch(dev, [logits[u.start_frame:u.end_frame] for u in finals], 29)
  want = eng.beam_search_decode_nbest(1, 16, hotwords=hw)
  assert [u.ids for u in finals] == [l[0][0] for l in want]
  assert [np.float32(u.logp).tobytes() for u in finals] == [np.float32(l[0][1]).tobytes() for l in want]
  assert [_key(u) for u in finals] != [_key(u) for u in plain] and sum(hw.score(u.ids)[1] for u in finals) > 0


def test_cli_stream_with_hotwords(dev, golden_dir, tmp_path, capsys, monkeypatch):
  from speecht_amd import transcription, vocabulary
  from speecht_amd.hotwords import Hotwords
  from speecht_amd.speech_input import SingleInputLoader
  from speecht_amd.speech_model import Session, Wav2LetterModel
  from speecht_amd.streaming import StreamBeam, stream_audio
  loader = importlib.machinery.SourceFileLoader('speecht_cli_stream_hotwords_gpu', os.path.join(ROOT, 'speecht-cli'))
  spec = importlib.util.spec_from_loader('speecht_cli_stream_hotwords_gpu', loader)
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
  seconds = len(samples) / float(rate) + 1.0
  with Session(dev) as sess:
    model.init_session(sess)
    model.saver.save(sess, str(train / 'run' / 'speechT'), global_step=model.global_step)
    plain, _ = stream_audio(model.engine, pieces, rate, 128, 'running', None, max_piece=per, beam=StreamBeam(beam_width=16, max_seconds=seconds))
    text = vocabulary.ids_to_sentence(plain)
    phrase = (text[:4].strip() or 'the')
    beam = StreamBeam(beam_width=16, max_seconds=seconds, hotwords=Hotwords([phrase, 'zebra'], 2.0))
    ids, _ = stream_audio(model.engine, pieces, rate, 128, 'running', None, max_piece=per, beam=beam)
  cwd = tmp_path / 'cwd'
  cwd.mkdir()
  monkeypatch.chdir(cwd)
  capsys.readouterr()
  # no --beam-width: hotwords alone ask for the beam search, beam 16 as in `transcribe`
  code = cli.main(['stream', '--train-dir', str(train), '--run-name', 'run', '--device', dev, '--hotword', phrase, '--hotword', 'zebra',
                   '--hotword-weight', '2.0', flac])
  lines = capsys.readouterr().out.splitlines()
  assert code == 0 and lines[-1] == '{}\t{}'.format(flac, vocabulary.ids_to_sentence(ids))
  fields = [l.split('\t') for l in lines[:-1]]
  assert fields and all(len(f) == 3 for f in fields)               # the beam search's partial lines: seconds, hypothesis, final characters
  assert sorted(os.listdir(str(cwd))) == []
