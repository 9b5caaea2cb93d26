"""Word times and confidences for the finals of live streams on the GPU, in the order the layers stack.
1. The C ABI (st_stream_keep_f32, st_ctc_align_ring_f32, st_ctc_word_conf_ring_f32) behind the endpoint kernel, driven by
   tests/endpoint_cases.py: every step keeps its rows in a ring of exactly st_stream_keep_rows(M, max_rows) rows, and every final the
   step closes is aligned and scored from the ring -- spans, states, score bits, status, log_prob and log_conf bits equal
   st_ctc_align_host / st_ctc_word_conf_host on the utterance's rows alone, for every cut; the situations a ring can get wrong are
   counted; label lengths at the dispatch edges, labels that do not fit, 32 classes, a reused slot, bad jobs and bad arguments.
2. StreamingRecognizer(words=FinalWords(...)): every final's spans, align_score, confidence and words are the host forms' on the rows
   the step returned, the same for every chunking and beside other streams; a long step; words=None launches what it launched before;
   `speecht-cli stream --endpoint --timestamps --confidence`."""
import ctypes

import numpy as np
import pytest

from tests import endpoint_cases as EC
from tests import endpoint_oracle as EO
from tests.test_gpu_endpoint import DeviceStep, _beam, _endpointing, _key, _stream

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

GUARD = 64
NEG_INF = float('-inf')


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


@pytest.fixture(scope='module')
def tiny(dev):
  from speecht_amd.engine import Wav2LetterEngine
  layers, params = EC.recognizer_model()
  eng = Wav2LetterEngine(layers, device=dev)
  eng.set_weights(params)
  return eng


def _ptr(t):
  return ctypes.c_void_p(t.data_ptr())


def _np(a):
  return a.ctypes.data_as(ctypes.c_void_p)


def _runs(ids, space):
  from speecht_amd.alignment import word_runs
  return word_runs(ids, space) if space >= 0 else []


# ---- the host forms on one utterance's rows alone: the reference of everything below -------------------------------------------------

def host_align(rows, ids):
  """st_ctc_align_host on rows [n, C] -> (spans [L, 2], states [n], score as float32 bits, status)."""
  from speecht_amd import _lib
  lib = _lib.load()
  n, C = rows.shape
  frames, L = max(n, 1), len(ids)
  x = np.zeros((frames, C), np.float32)
  x[:n] = rows
  lab, offs, lens = np.asarray(list(ids) + [0], np.int32), np.asarray([0, L], np.int32), np.asarray([n], np.int32)
  spans, states, score, status = np.full((L + 1, 2), -9, np.int32), np.full(frames, -9, np.int32), np.zeros(1, np.float32), np.zeros(1, np.int32)
  ws = np.zeros(int(lib.st_ctc_align_ws(1, frames, L)) // 8 + 2, np.float64)
  _lib.call('st_ctc_align_host', _np(x), 1, frames, C, _np(lab), _np(offs), _np(lens), L, _np(spans), _np(states), _np(score), _np(status),
            _np(ws), ws.nbytes)
  return spans[:L], states[:n], score.view(np.int32)[0], int(status[0])


def host_conf(rows, ids, space):
  """st_ctc_word_conf_host on rows [n, C] -> (log_prob bits, log_conf bits [W], status)."""
  from speecht_amd import _lib
  lib = _lib.load()
  n, C = rows.shape
  frames, L = max(n, 1), len(ids)
  x = np.zeros((frames, C), np.float32)
  x[:n] = rows
  runs = _runs(ids, space)
  W = len(runs)
  lab, offs, lens = np.asarray(list(ids) + [0], np.int32), np.asarray([0, L], np.int32), np.asarray([n], np.int32)
  spans = np.asarray([(0, a, e) for a, e in runs] + [(0, 0, 0)], np.int32)
  log_prob, log_conf, status = np.zeros(1, np.float64), np.zeros(W + 1, np.float64), np.zeros(1, np.int32)
  ws = np.zeros(int(lib.st_ctc_word_conf_ws(1, frames, L, 1 + W)) // 8 + 2, np.float64)
  _lib.call('st_ctc_word_conf_host', _np(x), 1, frames, C, _np(lab), _np(offs), _np(lens), L, space, _np(spans), W, _np(log_prob), _np(log_conf),
            _np(status), _np(ws), ws.nbytes)
  return log_prob.view(np.int64)[0], log_conf[:W].view(np.int64).copy(), int(status[0])


class Ring:
  """The ring of S streams and the two lattices on it, through the C ABI.  The ring starts as NaN with guard words behind it; every
  output of a call is pre-filled and has guard words behind it."""

  def __init__(self, dev, S, C, M, max_rows, cap=None):
    from speecht_amd import _lib
    self.lib, self.raw, self.dev, self.S, self.C, self.M = _lib, _lib.load(), dev, S, C, M
    self.cap = int(self.raw.st_stream_keep_rows(M, max_rows)) if cap is None else cap
    assert self.cap == M + max_rows or cap is not None            # exactly what the contract says: no slack
    self.ring = torch.full((S * self.cap * 32 + GUARD,), float('nan'), dtype=torch.float32, device=dev)
    self.ring[S * self.cap * 32:] = 77.0

  def keep(self, buf, pitch, rows, n_rows):
    self.lib.call('st_stream_keep_f32', _ptr(buf), pitch, self.C, _ptr(rows), n_rows, self.S, _ptr(self.ring), self.cap, None)

  def guard_intact(self):
    return bool((self.ring[self.S * self.cap * 32:] == 77.0).all())

  def _table(self, jobs, labels):
    offs = np.zeros(len(jobs) + 1, np.int32)
    offs[1:] = np.cumsum([len(l) for l in labels])
    ids = np.asarray([i for l in labels for i in l] + [0], np.int32)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.dev)
    return to(np.asarray(jobs, np.int32).reshape(-1)), to(ids), to(offs), offs, max([len(l) for l in labels] + [0])

  def align(self, jobs, labels, max_rows, with_states=True):
    """-> per job (spans [L, 2], states [max_rows], score bits, status)."""
    J = len(jobs)
    d_jobs, d_ids, d_offs, offs, max_len = self._table(jobs, labels)
    N = int(offs[-1])
    fill = lambda n: torch.full((n + GUARD,), -77, dtype=torch.int32, device=self.dev)
    spans, states, score, status = fill(2 * N), fill(J * max_rows), fill(J), fill(J)
    need = int(self.raw.st_ctc_align_ws(J, max_rows, max_len))
    ws = torch.empty(need // 4 + 4, dtype=torch.int32, device=self.dev)
    self.lib.call('st_ctc_align_ring_f32', _ptr(self.ring), self.S, self.cap, self.C, _ptr(d_jobs), J, max_rows, _ptr(d_ids), _ptr(d_offs),
                  max_len, _ptr(spans), _ptr(states) if with_states else None, _ptr(score), _ptr(status), _ptr(ws), need, None)
    torch.cuda.synchronize()
    spans, states, score, status = (t.cpu().numpy() for t in (spans, states, score, status))
    assert (spans[2 * N:] == -77).all() and (states[J * max_rows:] == -77).all() and (score[J:] == -77).all() and (status[J:] == -77).all()
    if not with_states:
      assert (states == -77).all()
    return [(spans[2 * offs[j]:2 * offs[j + 1]].reshape(-1, 2), states[j * max_rows:(j + 1) * max_rows], score[j], int(status[j]))
            for j in range(J)]

  def conf(self, jobs, labels, max_rows, space):
    """-> per job (log_prob bits, log_conf bits [W_j], status)."""
    J = len(jobs)
    d_jobs, d_ids, d_offs, offs, max_len = self._table(jobs, labels)
    runs = [_runs(l, space) for l in labels]
    W = sum(len(r) for r in runs)
    d_spans = torch.from_numpy(np.asarray([(j, a, e) for j, r in enumerate(runs) for a, e in r] + [(0, 0, 0)], np.int32)).to(self.dev)
    log_prob = torch.full((J + GUARD,), 7.0, dtype=torch.float64, device=self.dev)
    log_conf = torch.full((W + GUARD,), 7.0, dtype=torch.float64, device=self.dev)
    status = torch.full((J + GUARD,), -77, dtype=torch.int32, device=self.dev)
    need = int(self.raw.st_ctc_word_conf_ws(J, max_rows, max_len, J + W))
    ws = torch.empty(need // 4 + 4, dtype=torch.int32, device=self.dev)
    self.lib.call('st_ctc_word_conf_ring_f32', _ptr(self.ring), self.S, self.cap, self.C, _ptr(d_jobs), J, max_rows, _ptr(d_ids), _ptr(d_offs),
                  max_len, space, _ptr(d_spans), W, _ptr(log_prob), _ptr(log_conf), _ptr(status), _ptr(ws), need, None)
    torch.cuda.synchronize()
    log_prob, log_conf, status = log_prob.cpu().numpy(), log_conf.cpu().numpy(), status.cpu().numpy()
    assert (log_prob[J:] == 7.0).all() and (log_conf[W:] == 7.0).all() and (status[J:] == -77).all()
    first = np.concatenate([[0], np.cumsum([len(r) for r in runs])])
    return [(log_prob[:J].view(np.int64)[j], log_conf[first[j]:first[j + 1]].view(np.int64), int(status[j])) for j in range(J)]


def check_jobs(ring, jobs, labels, rows_of, max_rows, space):
  """Every job's ring alignment and (with a space class and C <= 30) ring confidences against the host forms on ``rows_of(j)``."""
  got = ring.align(jobs, labels, max_rows)
  conf = ring.conf(jobs, labels, max_rows, space) if space >= 0 and ring.C <= 30 else None
  for j, (job, ids) in enumerate(zip(jobs, labels)):
    rows = rows_of(j)
    n = len(rows)
    spans, states, score, status = host_align(rows, ids)
    where = (job, ids)
    assert got[j][3] == status and got[j][2] == score, where
    assert (got[j][0] == spans).all() and (got[j][1][:n] == states).all() and (got[j][1][n:] == -2).all(), where
    if conf is not None:
      log_prob, log_conf, cstatus = host_conf(rows, ids, space)
      assert conf[j][2] == cstatus == status and conf[j][0] == log_prob and (conf[j][1] == log_conf).all(), where
  return got


# ---- 1. the ring behind the endpoint kernel -------------------------------------------------------------------------------------------

RING_SITUATIONS = ('wraps', 'length_with_rows_behind', 'ends_on_last_row', 'end_without_rows', 'two_finals_one_stream',
                   'streams_of_different_lengths', 'discard_between_finals')


class KeepAndAlign:
  """`on_step` of tests.endpoint_cases.drive behind a `DeviceStep`: the step's rows go to the ring, and the finals the step closed --
  with their greedy ids -- are aligned and scored from the ring, all finals of the step in one call, and held to the host forms on
  logits[s][u0:end]."""

  def __init__(self, dev, step, logits, S, C, space_id, M, max_rows, ring=None):
    self.step, self.logits, self.C, self.space, self.M, self.max_rows = step, logits, C, space_id, M, max_rows
    self.ring = ring or Ring(dev, S, C, M, max_rows)
    self.seen = {name: 0 for name in RING_SITUATIONS}
    self.finals, self.words, self.history = 0, 0, {}

  def on_step(self, k, plan, out, table):
    ring, cap = self.ring, self.ring.cap
    ring.keep(self.step.buf, EC.PITCH, self.step.rows, self.step.n_rows)
    jobs, labels = [], []
    for s, (a, b, _, _, finishing) in plan.items():
      mine = 0
      for e in out.events[s].tolist():
        if e[0] == 0:
          break
        hist = self.history.setdefault(s, [])
        if e[0] in EO.FINAL_KINDS:
          u0, end = e[1], e[2]
          jobs.append((s, u0, end - u0))
          labels.append(EO.collapse(EO.argmax_rows(self.logits[s][u0:end], self.C)[0], self.C - 1))
          mine += 1
          self.seen['wraps'] += u0 % cap + (end - u0) > cap
          self.seen['length_with_rows_behind'] += e[0] == EO.LENGTH and end - u0 == self.M and b > end
          self.seen['ends_on_last_row'] += b > a and end == b
          self.seen['end_without_rows'] += e[0] == EO.END and a == b
          self.seen['discard_between_finals'] += len(hist) >= 2 and hist[-1] == EO.DISCARD and any(h in EO.FINAL_KINDS for h in hist[:-1])
        hist.append(e[0])
      self.seen['two_finals_one_stream'] += mine >= 2
    if not jobs:
      return
    self.seen['streams_of_different_lengths'] += len({j[0] for j in jobs}) >= 2 and len({j[2] for j in jobs}) >= 2
    max_rows = max(j[2] for j in jobs)
    check_jobs(ring, jobs, labels, lambda j: self.logits[jobs[j][0]][jobs[j][1]:jobs[j][1] + jobs[j][2]], max_rows, self.space)
    self.finals += len(jobs)
    self.words += sum(len(_runs(l, self.space)) for l in labels)


def _drive(dev, seed, C, R, L, M, cuts, S=5, T=120, ring=None, **kw):
  space_id = C - 2
  logits, lens = EC.make_streams(seed, S, C, space_id, R, L, M, T=T)
  step = DeviceStep(dev, C, space_id, R, L, M, S)
  keeper = KeepAndAlign(dev, step, logits, S, C, space_id, M, max(cuts) + 3, ring=ring)
  EC.drive(step, logits, lens, C, space_id, R, L, M, cuts, on_step=keeper.on_step, **kw)
  assert keeper.ring.guard_intact()
  return keeper


@pytest.mark.parametrize('plan', [0, 2, 3, 4, 5], ids=lambda i: 'cuts{}'.format(i))
@pytest.mark.parametrize('C', [5, 29])
@pytest.mark.parametrize('RLM', [(2, 3, 9), (5, 7, 40)], ids=lambda p: 'R{}-L{}-M{}'.format(*p))
def test_ring_finals_equal_the_host_forms_for_every_cut(dev, RLM, C, plan):
  from speecht_amd._lib import launch_trace
  cuts = EC.cut_plans(5)[plan]
  with launch_trace() as tr:
    keeper = _drive(dev, 7 * C + plan, C, *RLM, cuts, sit_out=plan == 5, finish_apart=(0,) if plan == 5 else ())
  assert keeper.finals >= 5 and keeper.words >= 3, (keeper.finals, keeper.words)
  names = {l.split(' ')[0].split('<')[0] for l in tr.lines}
  assert {'stream_keep', 'ctc_align_ring', 'ctc_word_conf_ring'} <= names, names
  if RLM[2] == 9 and max(cuts) <= 10:
    assert keeper.seen['wraps'] > 0                                 # a ring of about 20 rows under 117 frames


def test_ring_meets_every_situation(dev):
  total = {name: 0 for name in RING_SITUATIONS}
  for i, (seed, C, cuts) in enumerate(((1, 5, [2] * 5), (2, 29, [7] * 5), (3, 5, [10] * 5), (4, 29, [10, 1, 2, 7, 10]), (5, 5, [7] * 5))):
    keeper = _drive(dev, seed, C, 2, 3, 9, cuts, sit_out=i != 2, finish_apart=(0, 1) if i < 3 else ())
    for name, n in keeper.seen.items():
      total[name] += n
  assert all(total[name] > 0 for name in RING_SITUATIONS), total


def test_a_reused_slot_needs_no_clearing(dev):
  """The same ring under a second set of streams, whose frames count from 0 again: their finals are right, the old rows never show."""
  first = _drive(dev, 11, 29, 2, 3, 9, [7] * 5)
  second = _drive(dev, 12, 29, 2, 3, 9, [7] * 5, ring=first.ring)
  assert second.finals >= 5 and not torch.isnan(first.ring.ring[:32 * first.ring.cap]).all()


def _kept(dev, C, n, start, M, seed, chunk=64):
  """One utterance of n rows, frames start .. start + n - 1 of stream 1 of 2, kept in passes of ``chunk`` rows -> (ring, rows)."""
  rng = np.random.default_rng(seed)
  x = (rng.standard_normal((n, C)) * 2.0).astype(np.float32)
  ring = Ring(dev, 2, C, M, chunk)
  for at in range(0, n, chunk):
    part = x[at:at + chunk]
    buf = np.full((len(part), 40), EC.POISON, np.float32)
    buf[:, :C] = part
    rows = np.stack([np.ones(len(part)), start + at + np.arange(len(part))], axis=1).astype(np.int32)
    ring.keep(torch.from_numpy(buf).to(dev), 40, torch.from_numpy(rows).to(dev), len(part))
  return ring, x


def _label(rng, L, C, space):
  """L ids without adjacent repeats (they fit L rows), a space now and then."""
  out = []
  for i in range(L):
    c = space if space >= 0 and i % 7 == 5 else int(rng.integers(0, C - 1))
    while out and c == out[-1]:
      c = int(rng.integers(0, C - 1))
    out.append(c)
  return out


@pytest.mark.parametrize('L', [0, 1, 31, 32])
def test_label_lengths_at_the_dispatch_edges(dev, L):
  C, space, n, M = 29, 27, 70, 80
  ring, x = _kept(dev, C, n, start=100, M=M, seed=L)              # cap 144: frames 100 .. 169 wrap
  rng = np.random.default_rng(100 + L)
  jobs = [(1, 100, n), (1, 100 + 5, n - 5), (1, 100, 33)]
  labels = [_label(rng, L, C, space) for _ in jobs]
  got = check_jobs(ring, jobs, labels, lambda j: x[jobs[j][1] - 100:jobs[j][1] - 100 + jobs[j][2]], n, space)
  assert all(g[3] == 0 for g in got)
  ring.align(jobs, labels, n, with_states=False)                    # states may be null


def test_the_longest_label_on_700_rows(dev):
  C, space, n, M = 29, 27, 700, 700
  ring, x = _kept(dev, C, n, start=500, M=M, seed=3)              # cap 764: frames 500 .. 1199 wrap
  label = _label(np.random.default_rng(5), 511, C, space)
  got = check_jobs(ring, [(1, 500, n)], [label], lambda j: x, n, space)
  assert got[0][3] == 0 and (got[0][0] >= 0).all()


def test_a_label_that_does_not_fit_and_bad_jobs_get_a_status(dev):
  C, space, n, M = 29, 27, 40, 40
  ring, x = _kept(dev, C, n, start=90, M=M, seed=9)
  jobs = [(1, 90, 3), (1, 90, 3), (1, 90, 0), (1, 90, 0), (-1, 90, 5), (2, 90, 5), (1, -1, 5), (1, 90, -1), (1, 90, n + 1), (1, 100, 20)]
  labels = [[1, 2, 3, 4], [1, 1, 2], [], [3], [1, 27, 2], [1, 27, 2], [1, 27, 2], [1, 27, 2], [1, 27, 2], [4, 27, 5]]
  rows = lambda j: x[jobs[j][1] - 90:jobs[j][1] - 90 + max(jobs[j][2], 0)] if 0 <= jobs[j][0] < 2 and jobs[j][1] >= 90 and 0 <= jobs[j][2] <= n else None
  got = ring.align(jobs, labels, n)
  conf = ring.conf(jobs, labels, n, space)
  nan = lambda bits: bool(np.isnan(bits.view(np.float64)).all())
  for j in (0, 1, 3, 4, 5, 6, 7, 8):                                # does not fit (too long, a repeat, no rows) or no such job
    assert got[j][3] != 0 and conf[j][2] != 0, j
    assert (got[j][0] == -1).all() and (got[j][1] == -2).all() and np.int32(got[j][2]).view(np.float32) == NEG_INF, j
    assert np.int64(conf[j][0]).view(np.float64) == NEG_INF and nan(conf[j][1]), j
  for j in (0, 1, 3):                                               # ... the first three as the dense entry points define it
    assert host_align(rows(j), labels[j])[3] != 0 and host_conf(rows(j), labels[j], space)[2] != 0
  for j in (2, 9):                                                  # the good jobs beside them
    spans, states, score, status = host_align(rows(j), labels[j])
    log_prob, log_conf, _ = host_conf(rows(j), labels[j], space)
    assert got[j][3] == status == 0 and got[j][2] == score and (got[j][0] == spans).all() and (got[j][1][:len(states)] == states).all()
    assert conf[j][0] == log_prob and (conf[j][1] == log_conf).all()
  assert ring.guard_intact()


def test_32_classes_for_the_alignment(dev):
  C, n, M = 32, 50, 60
  ring, x = _kept(dev, C, n, start=70, M=M, seed=2)               # cap 124: frames 70 .. 119, then a second job that wraps
  rng = np.random.default_rng(8)
  jobs = [(1, 70, n), (1, 81, 30)]
  labels = [_label(rng, 20, C, -1), _label(rng, 9, C, -1)]
  got = check_jobs(ring, jobs, labels, lambda j: x[jobs[j][1] - 70:jobs[j][1] - 70 + jobs[j][2]], n, -1)
  assert all(g[3] == 0 for g in got)


def test_entry_points_refuse_bad_requests_without_a_launch(dev):
  from speecht_amd import _lib
  from speecht_amd._lib import launch_trace
  lib = _lib.load()
  z = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device=dev)
  S, cap, C, T = 2, 12, 29, 8
  ring, buf, rows, jobs, ids, offs = z(S * cap * 32, torch.float32), z(4 * 32, torch.float32), z(8), z(3), z(4), z(2)
  spans, score, status, lp, lc, wspans = z(8), z(1, torch.float32), z(1), z(1, torch.float64), z(2, torch.float64), z(3)
  need_a, need_c = int(lib.st_ctc_align_ws(1, T, 3)), int(lib.st_ctc_word_conf_ws(1, T, 3, 2))
  ws = z(max(need_a, need_c) // 4 + 4)
  ok = dict(ring=_ptr(ring), cap=cap, C=C, jobs=_ptr(jobs), n_jobs=1, T=T, ids=_ptr(ids), max_len=3, out=_ptr(spans), ws=_ptr(ws),
            buf=_ptr(buf), rows=_ptr(rows), n_rows=4, pitch=32, space=27)

  def keep(**kw):
    a = dict(ok, **kw)
    return lib.st_stream_keep_f32(a['buf'], a['pitch'], a['C'], a['rows'], a['n_rows'], S, a['ring'], a['cap'], None)

  def align(bytes_=need_a, **kw):
    a = dict(ok, **kw)
    return lib.st_ctc_align_ring_f32(a['ring'], S, a['cap'], a['C'], a['jobs'], a['n_jobs'], a['T'], a['ids'], _ptr(offs), a['max_len'], a['out'],
                                     None, _ptr(score), _ptr(status), a['ws'], bytes_, None)

  def conf(bytes_=need_c, **kw):
    a = dict(ok, **kw)
    return lib.st_ctc_word_conf_ring_f32(a['ring'], S, a['cap'], a['C'], a['jobs'], a['n_jobs'], a['T'], a['ids'], _ptr(offs), a['max_len'],
                                         a['space'], _ptr(wspans), 1, _ptr(lp), _ptr(lc), _ptr(status), a['ws'], bytes_, None)

  with launch_trace() as tr:
    for kw, text in ((dict(buf=None), 'null'), (dict(rows=None), 'null'), (dict(ring=None), 'null'), (dict(cap=0), 'bad sizes'),
                     (dict(C=33), 'num_classes'), (dict(C=0), 'num_classes'), (dict(pitch=28), 'pitch'), (dict(n_rows=-1), 'bad sizes')):
      assert keep(**kw) != 0, kw
      assert text in lib.st_last_error().decode(), (kw, lib.st_last_error().decode())
    assert keep(n_rows=0) == 0                                      # valid, and launches nothing
    for kw, text in ((dict(ring=None), 'null'), (dict(jobs=None), 'null'), (dict(out=None), 'null'), (dict(ws=None), 'null'),
                     (dict(cap=0), 'bad ring'), (dict(n_jobs=0), 'bad ring'), (dict(T=0), 'bad ring'), (dict(C=33), 'num_classes'),
                     (dict(C=1), 'num_classes'), (dict(max_len=512), 'label length'), (dict(bytes_=need_a - 1), 'workspace too small')):
      assert align(**kw) != 0, kw
      assert text in lib.st_last_error().decode(), (kw, lib.st_last_error().decode())
    for kw, text in ((dict(ring=None), 'null'), (dict(jobs=None), 'null'), (dict(ws=None), 'null'), (dict(cap=0), 'bad ring'),
                     (dict(C=31), 'num_classes <= 30'), (dict(space=28), 'space_id'), (dict(space=-1), 'space_id'), (dict(n_jobs=0), 'n_jobs'),
                     (dict(max_len=512), 'max_label_len'), (dict(bytes_=need_c - 1), 'workspace too small')):
      assert conf(**kw) != 0, kw
      assert text in lib.st_last_error().decode(), (kw, lib.st_last_error().decode())
  assert tr.lines == []
  torch.cuda.synchronize()


# ---- 2. the recogniser ---------------------------------------------------------------------------------------------------------------

def _words():
  from speecht_amd.streaming import FinalWords
  return FinalWords(timestamps=True, confidence=True)


def _word_key(u):
  return (_key(u), None if u.spans is None else u.spans.tobytes(), None if u.align_score is None else np.float32(u.align_score).tobytes(),
          None if u.confidence is None else (np.float64(u.confidence['log_prob']).tobytes(), np.asarray(u.confidence['words']).tobytes()),
          repr(u.words))


def _check_final_words(finals, logits):
  """Every final's new fields against the host forms on the returned rows [start_frame, end_frame) with the final's ids."""
  from speecht_amd import alignment
  from speecht_amd.engine_decode import MAX_ALIGN_LABELS
  some = 0
  for u in finals:
    rows = logits[u.start_frame:u.end_frame]
    if len(u.ids) == 0:
      assert u.words == [] and u.spans.shape == (0, 2) and u.align_score is None and u.confidence is None
      continue
    assert len(u.ids) <= MAX_ALIGN_LABELS
    spans, _, score, status = host_align(rows, u.ids)
    log_prob, log_conf, cstatus = host_conf(rows, u.ids, 27)
    if status != 0:
      assert cstatus != 0 and u.spans is None and u.align_score is None and u.confidence is None and u.words is None
      continue
    some += 1
    assert u.spans.dtype == np.int32 and (u.spans == spans).all() and np.float32(u.align_score).view(np.int32) == score
    assert np.float64(u.confidence['log_prob']).view(np.int64) == log_prob
    probs = np.exp(log_conf.view(np.float64))
    assert np.asarray(u.confidence['words']).tobytes() == probs.tobytes() and ((probs > 0) & (probs <= 1)).all()
    runs = alignment.word_runs(u.ids)
    assert len(u.words) == len(runs) == len(probs)
    for w, (a, e), p in zip(u.words, runs, probs):                  # the times those spans imply: 20 ms per row of this model
      assert w['start'] == round((u.start_frame + int(spans[a][0])) * 0.02, 4) and w['end'] == round((u.start_frame + int(spans[e - 1][1])) * 0.02, 4)
      assert u.start_frame * 0.02 - 5e-5 <= w['start'] < w['end'] <= u.end_frame * 0.02 + 5e-5   # (times are rounded to 0.1 ms)
      assert w['confidence'] == round(float(p), 6) and len(w['word']) == e - a
  return some


@pytest.mark.parametrize('which', ['greedy', 'free', 'lm'])
def test_recognizer_finals_carry_the_host_forms_words_for_every_cut(dev, tiny, which):
  from speecht_amd._lib import launch_trace
  from speecht_amd.streaming import StreamingRecognizer
  xa, xb = EC.recognizer_features('a'), EC.recognizer_features('b')[:500]
  make = lambda S, words=True: StreamingRecognizer(tiny, S, max_chunk_frames=64, beam=_beam(which), endpoint=_endpointing(),
                                                   words=_words() if words else None)
  rec = make(1)
  with launch_trace() as tr:
    finals, logits, seen, _ = _stream(rec, rec.open(), xa, 64)
  names = [l.split(' ')[0].split('<')[0] for l in tr.lines]
  assert 'stream_keep' in names and 'ctc_align_ring' in names and 'ctc_word_conf_ring' in names
  assert len(finals) >= 3 and _check_final_words(finals, logits) >= 2
  assert any(u.kind == 'length' for u in finals) and any(u.kind == 'silence' for u in finals)
  # the same input cut at other chunk sizes, and beside a second stream that goes at its own pace: identical finals, the new fields too
  for chunk in (1, 7):
    rec2 = make(1)
    finals2, logits2, _, _ = _stream(rec2, rec2.open(), xa, chunk)
    assert logits2.tobytes() == logits.tobytes() and [_word_key(u) for u in finals2] == [_word_key(u) for u in finals], chunk
  duo = make(2)
  a, b = duo.open(), duo.open()
  finals3, logits3, _, side = _stream(duo, a, xa, 64, others={b: (xb, 50)})
  assert logits3.tobytes() == logits.tobytes() and [_word_key(u) for u in finals3] == [_word_key(u) for u in finals]
  assert len(side[b][0]) >= 1 and _check_final_words(*side[b]) >= 1
  # without words: every existing field of every final and every partial is what it is with them
  plain = make(1, words=False)
  finals0, logits0, seen0, _ = _stream(plain, plain.open(), xa, 64)
  assert logits0.tobytes() == logits.tobytes() and seen0 == seen and [_key(u) for u in finals0] == [_key(u) for u in finals]
  assert all(u.spans is None and u.align_score is None and u.confidence is None and u.words is None for u in finals0)


def test_a_long_step_closes_finals_in_its_early_passes(dev, tiny):
  from speecht_amd.streaming import FinalWords, StreamingRecognizer
  xa = EC.recognizer_features('a')
  rec = StreamingRecognizer(tiny, 1, max_chunk_frames=64, endpoint=_endpointing(), words=_words())
  want, logits, _, _ = _stream(rec, rec.open(), xa, 64)
  long = StreamingRecognizer(tiny, 1, max_chunk_frames=64, endpoint=_endpointing(), words=_words())
  slot = long.open()
  r = long.step({slot: xa}, return_logits=True)                     # a dozen passes in one step
  assert len(r.finals[slot]) >= 2 and r.finals[slot][0].end_frame < len(r.logits[slot]) - long.ring_cap
  r2 = long.finish(slot, return_logits=True)
  got = r.finals[slot] + r2.finals[slot]
  assert [_word_key(u) for u in got] == [_word_key(u) for u in want]
  assert _check_final_words(got, np.concatenate([r.logits[slot], r2.logits[slot]])) >= 2
  # timestamps alone and confidences alone: the same values, the other fields None
  for stamps, conf in ((True, False), (False, True)):
    one = StreamingRecognizer(tiny, 1, max_chunk_frames=64, endpoint=_endpointing(), words=FinalWords(timestamps=stamps, confidence=conf))
    slot = one.open()
    part = one.step({slot: xa}).finals[slot] + one.finish(slot).finals[slot]
    assert [_key(u) for u in part] == [_key(u) for u in want]
    for u, w in zip(part, want):
      if w.words:
        assert (u.spans.tobytes() == w.spans.tobytes() and u.align_score == w.align_score and u.confidence is None) if stamps else \
            (u.confidence == w.confidence and u.spans is None and u.align_score is None)
        assert [x['word'] for x in u.words] == [x['word'] for x in w.words] and ('start' in u.words[0]) == stamps and ('confidence' in u.words[0]) == conf


def test_without_words_the_launches_are_the_old_ones(dev, tiny):
  from speecht_amd._lib import launch_trace
  from speecht_amd.streaming import StreamingRecognizer
  x = EC.recognizer_features('a')[:200]                             # silence: discards, no final
  for which, searches in (('greedy', 0), ('lm', 1)):
    traces, launches, recs = [], [], []
    for words in (None, _words()):
      rec = StreamingRecognizer(tiny, 1, max_chunk_frames=64, beam=_beam(which), endpoint=_endpointing(), words=words)
      slot = rec.open()
      rec.step({slot: x[:150]})
      with launch_trace() as tr:
        r = rec.step({slot: x[150:]})
      assert r.finals[slot] == []                                   # a pass that closes nothing
      traces.append([l.split(' ')[0].split('<')[0] for l in tr.lines])
      launches.append(rec.launches)
      recs.append(rec)
    plain, kept = recs
    assert plain.words is None and not hasattr(plain, 'ring') and 'stream_keep' not in traces[0]
    # feed, products with epilogues, advance + endpointer, with a search its log-softmax and a search + read-out per piece
    assert launches[0] == 1 + 22 + 2 + searches * (1 + 2 * plain.n_pieces)
    assert launches[1] == launches[0] + 1 and traces[1].count('stream_keep') == 1                 # one enqueue more, nothing else
    assert [n for n in traces[1] if n != 'stream_keep'] == traces[0]
    assert kept.dec_out.numel() == plain.dec_out.numel()


def test_cli_stream_with_word_times_and_confidences(dev, golden_dir, tmp_path, capsys, monkeypatch):
  import importlib.machinery
  import importlib.util
  import os
  from speecht_amd import transcription
  from speecht_amd.speech_input import SingleInputLoader
  from speecht_amd.speech_model import Session, Wav2LetterModel
  from speecht_amd.streaming import Endpointing, FinalWords, stream_audio
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  loader = importlib.machinery.SourceFileLoader('speecht_cli_stream_words_gpu', os.path.join(root, 'speecht-cli'))
  spec = importlib.util.spec_from_loader('speecht_cli_stream_words_gpu', loader)
  cli = importlib.util.module_from_spec(spec)
  loader.exec_module(cli)
  flac = os.path.join(golden_dir, '1089-134686-0037.flac')
  samples, rate = transcription.load_native(flac)
  duration = len(samples) / float(rate)
  model = Wav2LetterModel(SingleInputLoader(128), 128, 29)       # a checkpoint written the way test_gpu_stream.py does
  model.add_training_ops()
  model.add_decoding_ops()
  model.finalize(str(tmp_path / 'log'), 'r', 'record')
  model.init_seed = 1234
  train = tmp_path / 'train'
  (train / 'run').mkdir(parents=True)
  with Session(dev) as sess:
    model.init_session(sess)
    model.saver.save(sess, str(train / 'run' / 'speechT'), global_step=model.global_step)
    # the same stream through the API: the exact values the lines below print rounded (an untrained model's confidences are tiny)
    per = int(rate * 200 / 1000.0)
    finals, _ = stream_audio(model.engine, [samples[at:at + per] for at in range(0, len(samples), per)], rate, 128, 'running', max_piece=per,
                             endpoint=Endpointing(silence=0.1, lead=0.3, max_utterance=1.5), words=FinalWords(timestamps=True, confidence=True))
  exact = [w for u in finals for w in u.words]
  probs = [p for u in finals for p in u.confidence['words']]
  assert len(exact) >= 3 and all(0.0 < p <= 1.0 for p in probs) and all(0.0 <= w['start'] < w['end'] <= duration + 0.02 for w in exact)
  cwd = tmp_path / 'cwd'
  cwd.mkdir()
  monkeypatch.chdir(cwd)
  base = ['stream', '--train-dir', str(train), '--run-name', 'run', '--device', dev]
  for flag in ('--timestamps', '--confidence'):
    with pytest.raises(SystemExit) as e:
      cli.main(base + [flag, flac])
    assert e.value.code == 2 and '--endpoint' in capsys.readouterr().err
  code = cli.main(base + ['--endpoint', '--endpoint-silence', '0.1', '--endpoint-lead', '0.3', '--max-utterance', '1.5', '--timestamps',
                          '--confidence', flac])
  lines = capsys.readouterr().out.splitlines()
  assert code == 0 and lines[-1].startswith(flac + '\t')
  words, texts, pending = 0, [], None
  for line in lines[:-1]:
    f = line.split('\t')
    if f[0] == 'utt':
      assert pending is None or pending == []                       # the words of the final before were all printed
      pending = f[4].split()
      texts.append(f[4])
    elif f[0] == flac:
      w = exact[words]                                              # the line is that word, in the format of `transcribe --timestamps`
      assert f[1:] == ['{:.3f}'.format(w['start']), '{:.3f}'.format(w['end']), w['word'], '{:.4f}'.format(w['confidence'])]
      assert 0.0 <= float(f[1]) < float(f[2]) <= duration + 0.02 and 0.0 <= float(f[4]) <= 1.0
      assert pending and f[3] == pending.pop(0)
      words += 1
  assert pending == [] and words == len(exact) and len(texts) == len(finals) >= 2
  with pytest.raises(SystemExit):
    cli.main(['stream', '--help'])
  out = capsys.readouterr().out
  assert '--timestamps' in out and '--confidence' in out
  assert sorted(os.listdir(str(cwd))) == []
