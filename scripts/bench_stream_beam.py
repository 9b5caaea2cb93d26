#!/usr/bin/env python3
"""The beam search carried across steps (st_ctc_beam_stream_step / _read, StreamingRecognizer(beam=...)): what it costs.

  (a) offline   the whole-utterance entry points the frame loop is shared with -- top path and N best, beam 16 LM-free and beam 100
                with the synthetic 200 k / 1 M / 1 M trigram of scripts/bench_lm_decode.py, 16 x 1 501 frames -- in this build and,
                with --parent-lib, in the parent commit's library loaded beside it (same process, same buffers, alternating).
  (b) per frame the step entry point, 10 rows per stream and step at 1, 16 and 64 streams, against the offline kernel's time per
                frame on the same rows (its time / 1 501).
  (c) step      StreamingRecognizer.step with the beam search on against the same build's greedy step: full-size 80-mel model,
                200 ms per step; streams sustained in real time = streams * 0.2 s / step time.
  (d) read-out  st_ctc_beam_stream_read on the same streams after 500 and after 5 000 decoded frames, with the tail it walks.

The clock is that of scripts/bench_stream.py: host time around work that ends in a device synchronise, the forms alternating inside
every round, median and range of the rounds.  Writes profiles/stream_beam.json (--output)."""
import argparse, ctypes, json, os, sys, tempfile, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import bench_lm_decode as BL  # noqa: E402
from speecht_amd import _lib  # noqa: E402
from speecht_amd.engine import Wav2LetterEngine  # noqa: E402
from speecht_amd.language_model import LanguageModel  # noqa: E402
from speecht_amd.streaming import StreamBeam, StreamingRecognizer  # noqa: E402
from tests.workloads import synthetic_features, w2l_layers  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'stream_beam.json'))
ap.add_argument('--parent-lib', default=None, help="the parent commit's libspeecht_hip.so, for (a)")
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--streams', type=int, nargs='+', default=[1, 16, 64])
ap.add_argument('--unigrams', type=int, default=200000)
ap.add_argument('--bigrams', type=int, default=1000000)
ap.add_argument('--trigrams', type=int, default=1000000)
ap.add_argument('--parts', default='abcd')
a = ap.parse_args()
if not torch.cuda.is_available():
  sys.exit('bench_stream_beam.py needs a GPU')
dev = torch.device('cuda:0')
W4 = (0.8, 0.0, 2.3, -1000.0)
cf = lambda v: [ctypes.c_float(x) for x in v]
P = lambda t: ctypes.c_void_p(t.data_ptr())


def clock(fn, calls):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(calls):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / calls * 1e3


def spread(v):
  return dict(median=round(sorted(v)[len(v) // 2], 5), min=round(min(v), 5), max=round(max(v), 5))


text, words = BL.synthetic_arpa(1234, a.unigrams, a.bigrams, a.trigrams)
with tempfile.TemporaryDirectory() as d:
  path = os.path.join(d, 'synthetic.arpa')
  with open(path, 'w') as f:
    f.write(text)
  lm = LanguageModel(path)
del text
handle = lm.device_handle(dev)
lib = _lib.load()
T, B0 = 1501, 16
spelled = BL.spelled_logits(77, words[:5000], B0, T)              # [16, 1501, 29]
out = dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, model=dict(lm.info, synthetic_seed=1234),
           timing='host clock around work that ends in a device synchronise; the forms alternate inside every round')


def offline_engine(batch):
  eng = Wav2LetterEngine([(1, 1, 16, 29, False)], device=dev)
  eng.load_batch(np.zeros((batch, T, 16), dtype=np.float32), [T] * batch)
  eng.X[-1].interior().copy_(torch.as_tensor(np.stack([spelled[b % B0] for b in range(batch)])))
  eng.ctc_lens = torch.full((batch,), T, dtype=torch.int32, device=dev)
  eng._wait_uploads()
  return eng


def offline_calls(L, eng, n_best=10):
  """The four offline cases as closures over library L (this build's or the parent's)."""
  B = eng.dec_lens.numel()
  ws = eng._storage.view('beam_ws', lib.st_ctc_beam_ws(B, eng.t_out, 128) // 4 + 16, torch.int32)[0]
  nb = eng._storage.view('bench_nbest', B * n_best * (T + 2) + B + 16, torch.int32)[0]
  at = lambda first: ctypes.c_void_p(nb.data_ptr() + 4 * first)
  ref, lens, sp = eng.X[-1].ref, eng._ptr(eng.ctc_lens), eng.stream_ptr
  ids, dl, ds = eng._ptr(eng.dec_ids), eng._ptr(eng.dec_lens), eng._ptr(eng.dec_score)
  nbest_out = (at(0), T, at(B * n_best * T), at(B * n_best * T + B * n_best), at(B * n_best * T + 2 * B * n_best))
  return {
      'top_beam16_free': lambda: L.st_ctc_beam_search_decode_ex(ref, lens, 16, 1, ids, eng.t_out, dl, ds, P(ws), ws.numel() * 4, sp),
      'nbest_beam16_free': lambda: L.st_ctc_beam_search_decode_nbest(ref, lens, 16, 1, n_best, *nbest_out, P(ws), ws.numel() * 4, sp),
      'top_beam100_lm': lambda: L.st_ctc_beam_search_decode_lm(ref, lens, 100, 1, handle, *cf(W4), ids, eng.t_out, dl, ds, P(ws),
                                                               ws.numel() * 4, sp),
      'nbest_beam100_lm': lambda: L.st_ctc_beam_search_decode_lm_nbest(ref, lens, 100, 1, handle, *cf(W4), n_best, *nbest_out, P(ws),
                                                                        ws.numel() * 4, sp),
  }


# ---- (a) ----------------------------------------------------------------------------------------------------------------------
if 'a' in a.parts:
  eng = offline_engine(B0)
  mine = offline_calls(lib, eng)
  parent = None
  if a.parent_lib:
    pl = ctypes.CDLL(a.parent_lib)
    for name in ('st_ctc_beam_search_decode_ex', 'st_ctc_beam_search_decode_nbest', 'st_ctc_beam_search_decode_lm',
                 'st_ctc_beam_search_decode_lm_nbest'):
      getattr(pl, name).restype, getattr(pl, name).argtypes = _lib._SIGNATURES[name]
    parent = offline_calls(pl, eng)
  res = {}
  for case, fn in mine.items():
    assert fn() == 0, lib.st_last_error()
    t_new, t_old = [], []
    for _ in range(a.rounds):
      t_new.append(clock(fn, 2))
      if parent:
        t_old.append(clock(parent[case], 2))
    r = dict(ms=spread(t_new), us_per_frame=round(sorted(t_new)[len(t_new) // 2] * 1e3 / T, 3))
    if parent:
      ratios = [x / y for x, y in zip(t_new, t_old)]
      med = sorted(t_old)[len(t_old) // 2]
      r.update(parent_ms=spread(t_old), ratio_over_parent=spread(ratios), parent_own_spread=[round(min(t_old) / med, 4), round(max(t_old) / med, 4)])
      r['ratio_inside_parent_spread'] = bool(min(t_old) / med <= r['ratio_over_parent']['median'] <= max(t_old) / med)
    res[case] = r
    print(json.dumps({case: r}), flush=True)
  out['offline_16x1501'] = res
  del eng


# ---- the step entry point on prepared tables ----------------------------------------------------------------------------------
class Steps:
  """S streams of the spelled logits through the C ABI, `per` rows per stream and step; the tables and rows of every step are
  on the device before the clock starts."""

  def __init__(self, S, beam, with_lm, per=10, max_frames=1510, n_steps=150):
    self.S, self.beam, self.per, self.h = S, beam, per, handle if with_lm else None
    self.state = torch.zeros(S * lib.st_ctc_beam_stream_state_bytes(beam, int(with_lm)) // 8, dtype=torch.int64, device=dev)
    self.pool = torch.empty(S * lib.st_ctc_beam_stream_pool_bytes(max_frames, beam) // 8, dtype=torch.int64, device=dev)
    self.max_frames = max_frames
    self.ws_bytes = lib.st_ctc_beam_stream_ws(S * per)
    self.ws = torch.empty(self.ws_bytes // 4, dtype=torch.float32, device=dev)
    self.tail = torch.zeros(S * 512, dtype=torch.int32, device=dev)
    self.result = torch.zeros(S * 4, dtype=torch.int32, device=dev)
    self.k, self.n_steps = 0, n_steps
    pad = np.zeros((B0, T, 32), np.float32)
    pad[:, :, :29] = spelled
    self.bufs, self.rows, self.tables = [], [], []
    for k in range(n_steps):
      self.bufs.append(torch.from_numpy(np.concatenate([pad[s % B0, k * per:(k + 1) * per] for s in range(S)])).to(dev))
      self.rows.append(torch.tensor([(s, k * per + j) for s in range(S) for j in range(per)], dtype=torch.int32, device=dev))
      self.tables.append(torch.tensor([(s * per, per, -1, int(k == 0)) for s in range(S)], dtype=torch.int32, device=dev))

  def step(self, frame0=None):
    k = self.k % self.n_steps
    table = self.tables[k] if (k or self.k == 0) else self.tables[1]        # (going round: the rows repeat, the search goes on)
    _lib.call('st_ctc_beam_stream_step', P(self.bufs[k]), 32, 29, P(self.rows[k]), P(table), self.S * self.per, self.S, self.beam, 1,
              self.h, *cf(W4), P(self.state), P(self.pool), self.max_frames, P(self.ws), self.ws_bytes, None)
    self.k += 1
    return table

  def read(self, table):
    _lib.call('st_ctc_beam_stream_read', P(table), self.S, self.beam, self.h, *cf(W4), P(self.state), P(self.pool), self.max_frames,
              P(self.tail), 512, P(self.result), None)


# ---- (b) ----------------------------------------------------------------------------------------------------------------------
if 'b' in a.parts:
  res = []
  for beam, with_lm, case in ((100, True, 'top_beam100_lm'), (16, False, 'top_beam16_free')):
    for S in a.streams:
      eng = offline_engine(S)
      off = offline_calls(lib, eng)[case]
      t_step, t_off = [], []
      for _ in range(a.rounds):
        st = Steps(S, beam, with_lm)
        st.step()                                                   # the reset step, outside the clock
        t_step.append(clock(st.step, 140) * 1e3 / 10)               # us per frame: 140 steps of 10 frames per stream
        t_off.append(clock(off, 2) * 1e3 / T)
        del st
      r = dict(beam=beam, lm=with_lm, streams=S, rows_per_step=10, step_us_per_frame=spread(t_step), offline_us_per_frame=spread(t_off),
               ratio_step_over_offline=spread([x / y for x, y in zip(t_step, t_off)]),
               state_bytes_per_stream=int(lib.st_ctc_beam_stream_state_bytes(beam, int(with_lm))))
      print(json.dumps(r), flush=True)
      res.append(r)
      del eng
  out['step_per_frame'] = res

# ---- (d) ----------------------------------------------------------------------------------------------------------------------
if 'd' in a.parts:
  S = 16
  st = Steps(S, 100, True, max_frames=5010)
  res = []
  for target in (500, 5000):
    while st.k * 10 < target:
      table = st.step()
      if st.k % 5 == 0:
        st.read(table)                                              # a live stream is read as it goes: the stable length moves on
    st.read(table)
    torch.cuda.synchronize()
    info = st.result.cpu().numpy().reshape(S, 4)
    t = [clock(lambda: st.read(table), 100) * 1e3 for _ in range(a.rounds)]
    r = dict(beam=100, lm=True, streams=S, decoded_frames=st.k * 10, read_us=spread(t), hypothesis_len=info[:, 0].tolist(),
             unstable_tail=(info[:, 0] - info[:, 1]).tolist())
    print(json.dumps(r), flush=True)
    res.append(r)
  out['read_out'] = res
  del st

# ---- (c) ----------------------------------------------------------------------------------------------------------------------
if 'c' in a.parts:
  NEW = 20
  eng = Wav2LetterEngine(w2l_layers(80), device='cuda:0')
  eng.init_xavier(42)
  res = []
  for S in a.streams:
    x = np.stack([synthetic_features(s, 4000, 80) for s in range(S)]).astype(np.float32)
    forms = {'greedy': None, 'beam100_lm': StreamBeam(lm=lm, max_seconds=120.0, max_tail=2048),
             'beam16_free': StreamBeam(beam_width=16, max_seconds=120.0, max_tail=2048)}
    recs, steps = {}, {}
    for name, beam in forms.items():
      rec = StreamingRecognizer(eng, S, max_chunk_frames=NEW, beam=beam)
      slots = [rec.open() for _ in range(S)]
      at = [0]

      def step(rec=rec, slots=slots, at=at):
        if at[0] + NEW > x.shape[1]:
          at[0] = 0
        rec.step({slots[s]: x[s, at[0]:at[0] + NEW] for s in range(S)})
        at[0] += NEW

      for _ in range(8):
        step()
      recs[name], steps[name] = rec, step
    t = {name: [] for name in forms}
    for _ in range(a.rounds):
      for name in forms:
        t[name].append(clock(steps[name], 20))
    r = dict(streams=S, new_frames_per_step=NEW, launches_per_step={n: recs[n].launches for n in forms})
    for name in forms:
      med = sorted(t[name])[len(t[name]) // 2]
      r[name] = dict(step_ms=spread(t[name]), streams_in_real_time=round(S * 0.2 / (med * 1e-3), 1))
      if name != 'greedy':
        r[name]['ratio_over_greedy'] = spread([p / q for p, q in zip(t[name], t['greedy'])])
    print(json.dumps(r), flush=True)
    res.append(r)
    del recs, steps
    torch.cuda.empty_cache()
  out['whole_step_80mel'] = res

os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
with open(a.output, 'w') as f:
  json.dump(out, f, indent=1)
  f.write('\n')
