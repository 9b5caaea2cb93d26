#!/usr/bin/env python3
"""Hotword biasing of the streaming beam searches (st_ctc_beam_stream_step_bias / _read_bias / _step_pieces_bias): what it costs.

  (a) existing  ``--existing LIB --label NAME --out FILE``: the unbiased st_ctc_beam_stream_step / _read / _step_pieces and the four
                offline beam entry points of ONE build of the library (this one's or the parent commit's), in a process of its own;
                the caller alternates processes of the two builds in one session and ``--combine FILE ... --out RECORD`` folds
                them into the record: per entry point the ratio of the medians over the processes and, beside it, the spread
                (max / min) of the baseline's own processes, inside which the ratio must lie -- the instantiations are unchanged.
  (b) biased    the biased step against the unbiased step of the same build on the same rows, per frame and per 200 ms step (10 rows
                per stream): 1 / 16 / 64 streams, beam 16 LM-free and beam 100 with the synthetic 200 k / 1 M / 1 M trigram of
                scripts/bench_lm_decode.py, 100 and 1 000 phrases (those of scripts/bench_hotwords.py).  The yardstick is the offline
                cost of biasing in profiles/hotwords.json.
  (c) read-out  st_ctc_beam_stream_read_bias against st_ctc_beam_stream_read on open streams, and the records' sizes.

HIP events around the calls on rows and tables that are on the device before the clock starts (the method of
scripts/bench_hotwords.py), the variants alternating inside every round; median (min, max) of the rounds.  Writes
profiles/stream_hotwords.json (--out), which carries the digest of the sources it ran."""
import argparse
import ctypes
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_hotwords import baseline_library, phrases_from  # noqa: E402
from bench_lm_decode import spelled_logits, synthetic_arpa  # noqa: E402
from bench_nbest import WEIGHTS, spread  # noqa: E402
from speecht_amd import _lib  # noqa: E402
from speecht_amd.build import source_digest  # noqa: E402
from speecht_amd.engine import Wav2LetterEngine  # noqa: E402
from speecht_amd.hotwords import Hotwords, HotwordSets  # noqa: E402
from speecht_amd.language_model import LanguageModel  # noqa: E402

STREAM = ('st_ctc_beam_stream_state_bytes', 'st_ctc_beam_stream_pool_bytes', 'st_ctc_beam_stream_ws', 'st_ctc_beam_stream_step',
          'st_ctc_beam_stream_read', 'st_ctc_beam_stream_step_pieces')
PER, STEPS, T, B0 = 10, 140, 1501, 16                            # rows per stream and step (200 ms), clocked steps, the shard's shape
P = lambda t: ctypes.c_void_p(t.data_ptr())
cf = lambda v: [ctypes.c_float(x) for x in v]


def events(fn, reps):
  """ms per call between HIP events (the stream the library calls run on: the default one)."""
  torch.cuda.synchronize()
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(reps):
    fn()
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b) / reps


class Inputs:
  """The rows and tables of STEPS + 1 steps of S streams, on the device."""

  def __init__(self, S, spelled, dev):
    pad = np.zeros((B0, T, 32), np.float32)
    pad[:, :, :29] = spelled
    self.S, self.bufs, self.rows, self.tables, self.pieces = S, [], [], [], []
    for k in range(STEPS + 1):
      self.bufs.append(torch.from_numpy(np.concatenate([pad[s % B0, k * PER:(k + 1) * PER] for s in range(S)])).to(dev))
      self.rows.append(torch.tensor([(s, k * PER + j) for s in range(S) for j in range(PER)], dtype=torch.int32, device=dev))
      table = [(s * PER, PER, -1, int(k == 0)) for s in range(S)]
      self.tables.append(torch.tensor(table, dtype=torch.int32, device=dev))
      self.pieces.append(torch.tensor(table + [(0, 0, -1, 0)] * S, dtype=torch.int32, device=dev))   # two pieces, the second unused


class Steps:
  """One search over an `Inputs`: library L (this build's or the baseline's), its model handle, and -- biased -- the tables and roots."""

  def __init__(self, L, inputs, beam, handle, dev, bias=None):
    self.L, self.x, self.beam, self.h, self.k = L, inputs, beam, handle, 0
    S, lm = inputs.S, int(handle is not None)
    self.max_frames = PER * (STEPS + 1)
    size = L.st_ctc_beam_stream_bias_state_bytes if bias else L.st_ctc_beam_stream_state_bytes
    self.state_bytes = int(size(beam, lm))
    self.state = torch.zeros(S * self.state_bytes // 8, dtype=torch.int64, device=dev)
    self.pool = torch.empty(S * L.st_ctc_beam_stream_pool_bytes(self.max_frames, beam) // 8, dtype=torch.int64, device=dev)
    self.ws_bytes = L.st_ctc_beam_stream_ws(S * PER)
    self.ws = torch.empty(self.ws_bytes // 4, dtype=torch.float32, device=dev)
    self.tail = torch.zeros(2 * S * 512, dtype=torch.int32, device=dev)
    self.result = torch.zeros(2 * S * 4, dtype=torch.int32, device=dev)
    self.bias, self.suffix = (), ''
    if bias:
      tabs, struct, roots = bias
      self.bias, self.suffix = (ctypes.byref(struct), P(roots)), '_bias'

  def _check(self, rc):
    if rc != 0:
      raise RuntimeError('a library call failed')

  def step(self):
    x, k = self.x, self.k
    self._check(getattr(self.L, 'st_ctc_beam_stream_step' + self.suffix)(
        P(x.bufs[k]), 32, 29, P(x.rows[k]), P(x.tables[k]), x.S * PER, x.S, self.beam, 1, self.h, *cf(WEIGHTS), P(self.state), P(self.pool),
        self.max_frames, P(self.ws), self.ws_bytes, None, *self.bias))
    self.k += 1

  def step_pieces(self):
    x, k = self.x, self.k
    self._check(getattr(self.L, 'st_ctc_beam_stream_step_pieces' + self.suffix)(
        P(x.bufs[k]), 32, 29, P(x.rows[k]), P(x.pieces[k]), 2, x.S * PER, x.S, self.beam, 1, self.h, *cf(WEIGHTS), P(self.state),
        P(self.pool), self.max_frames, P(self.ws), self.ws_bytes, P(self.tail), 512, P(self.result), None, *self.bias))
    self.k += 1

  def read(self):
    self._check(getattr(self.L, 'st_ctc_beam_stream_read' + self.suffix)(
        P(self.x.tables[1]), self.x.S, self.beam, self.h, *cf(WEIGHTS), P(self.state), P(self.pool), self.max_frames, P(self.tail), 512,
        P(self.result), None, *self.bias))

  def run(self, how):
    """The reset step outside the clock, then STEPS steps -> us per frame."""
    self.k = 0
    getattr(self, how)()
    return events(getattr(self, how), STEPS) * 1e3 / PER


def existing_runs(L, h, x, beam, dev):
  return {'stream_step': (Steps(L, x, beam, h, dev), 'step'), 'stream_step_pieces': (Steps(L, x, beam, h, dev), 'step_pieces')}


def measure_existing(L, handle, spelled, streams, rounds, dev):
  """One build's existing entry points -> {name: [samples]}: stream_step* in us per frame, stream_read in us per call, offline_* in ms
  per call of 16 x 1501 frames."""
  out = {}
  for S in streams:
    x = Inputs(S, spelled, dev)
    for kind, beam, h in (('lm_free_beam16', 16, None), ('lm_beam100', 100, handle)):
      runs = existing_runs(L, h, x, beam, dev)
      name = lambda what: '{}_{}_S{}'.format(what, kind, S)
      for what in runs:
        out[name(what)] = []
      out[name('stream_read')] = []
      for _ in range(rounds):
        for what, (st, how) in runs.items():
          out[name(what)].append(st.run(how))
        out[name('stream_read')].append(events(runs['stream_step'][0].read, 50) * 1e3)
      del runs
    del x
    torch.cuda.empty_cache()
  eng = Wav2LetterEngine([(1, 1, 16, 29, False)], device=dev)
  eng.load_batch(np.zeros((B0, T, 16), dtype=np.float32), [T] * B0)
  eng.X[-1].interior().copy_(torch.as_tensor(spelled))
  eng.ctc_lens = torch.full((B0,), T, dtype=torch.int32, device=dev)
  ws = eng._storage.view('beam_ws', L.st_ctc_beam_ws(B0, eng.t_out, 128) // 4 + 16, torch.int32)[0]
  nb = [torch.zeros(n, dtype=dt, device=dev) for n, dt in ((B0 * eng.t_out, torch.int32), (B0, torch.int32), (B0, torch.float32),
                                                           (B0, torch.int32))]
  eng._wait_uploads()
  torch.cuda.synchronize()
  top = (eng._ptr(eng.dec_ids), eng.t_out, eng._ptr(eng.dec_lens), eng._ptr(eng.dec_score), P(ws), ws.numel() * 4, None)
  lists = (P(nb[0]), eng.t_out, P(nb[1]), P(nb[2]), P(nb[3]), P(ws), ws.numel() * 4, None)
  logits, lens, w = eng.X[-1].ref, eng._ptr(eng.ctc_lens), cf(WEIGHTS)
  calls = {'offline_lm_free_beam16': lambda: L.st_ctc_beam_search_decode_ex(logits, lens, 16, 1, *top),
           'offline_lm_beam100': lambda: L.st_ctc_beam_search_decode_lm(logits, lens, 100, 1, handle, *w, *top),
           'offline_lm_free_beam16_nbest1': lambda: L.st_ctc_beam_search_decode_nbest(logits, lens, 16, 1, 1, *lists),
           'offline_lm_beam100_nbest1': lambda: L.st_ctc_beam_search_decode_lm_nbest(logits, lens, 100, 1, handle, *w, 1, *lists)}
  for k, fn in calls.items():
    assert fn() == 0, k
    out[k] = []
  for _ in range(rounds):
    for k, fn in calls.items():
      out[k].append(events(fn, 3))
  return out


def bench_py_values(directory, baseline_name):
  """bench.py's result lines, one file per process (parent_*.json the baseline's tree, mine_*.json this one's) -> the record's part."""
  import glob
  value = lambda path: json.loads([l for l in open(path) if l.startswith('{')][-1])['value']
  b = [value(f) for f in sorted(glob.glob(os.path.join(directory, 'parent_*.json')))]
  a = [value(f) for f in sorted(glob.glob(os.path.join(directory, 'mine_*.json')))]
  m, t = float(np.median(a)), float(np.median(b))
  return dict(command='bench.py --gpus 1 --steps 20 --warmup 5, one process per build and repeat, alternating', unit='utterances/s',
              this_build=a, baseline=b, baseline_name=baseline_name, ratio=round(m / t, 4),
              baseline_min_max_over_median=[round(min(b) / t, 4), round(max(b) / t, 4)], inside=bool(min(b) <= m <= max(b)))


def combine(files, record_path, baseline_name, bench_py=None):
  """Fold the per-process files of --existing into the record: the processes of a label give one median each."""
  by = {}
  for path in files:
    with open(path) as f:
      one = json.load(f)
    for k, v in one['samples'].items():
      by.setdefault(one['label'], {}).setdefault(k, []).append(float(np.median(v)))
  labels = sorted(by)
  assert baseline_name in labels and len(labels) == 2, labels
  mine = next(l for l in labels if l != baseline_name)
  res = {}
  for k in by[mine]:
    a, b = by[mine][k], by[baseline_name][k]
    m, t = float(np.median(a)), float(np.median(b))
    res[k] = dict(this_build=[round(v, 4) for v in a], baseline=[round(v, 4) for v in b], ratio=round(m / t, 4),
                  baseline_min_max_over_median=[round(min(b) / t, 4), round(max(b) / t, 4)], baseline_max_over_min=round(max(b) / min(b), 4),
                  this_build_max_over_min=round(max(a) / min(a), 4), inside=bool(min(b) / t <= m / t <= max(b) / t))
  with open(record_path) as f:
    rec = json.load(f)
  rec['baseline'] = baseline_name
  rec['existing_over_baseline'] = res
  rec['existing_method'] = ('one process per build and repeat, the two builds\' processes alternating in one session ({} each); every '
                            'process gives the median of its rounds, the ratio is that of the medians over the processes; '
                            'stream_step*: us per frame, stream_read: us per call, offline_*: ms per call of 16 x 1501 frames'
                            .format(len(by[mine][next(iter(by[mine]))])))
  if bench_py:
    rec['bench_py_over_baseline'] = bench_py_values(bench_py, baseline_name)
  with open(record_path, 'w') as f:
    json.dump(rec, f, indent=1)
    f.write('\n')
  print(json.dumps({k: (v['ratio'], v['baseline_min_max_over_median'], v['inside']) for k, v in res.items()}))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--unigrams', type=int, default=200000)
  ap.add_argument('--bigrams', type=int, default=1000000)
  ap.add_argument('--trigrams', type=int, default=1000000)
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--streams', type=int, nargs='+', default=[1, 16, 64])
  ap.add_argument('--weight', type=float, default=1.0)
  ap.add_argument('--existing', default=None, metavar='LIB', help='time the existing entry points of this libspeecht_hip.so only')
  ap.add_argument('--label', default='this build')
  ap.add_argument('--combine', nargs='+', default=None, metavar='FILE', help='fold the files of --existing runs into the record --out')
  ap.add_argument('--bench-py', default=None, metavar='DIR', help='--combine: also the result lines of bench.py runs of the two trees')
  ap.add_argument('--baseline-name', default='parent commit')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stream_hotwords.json'))
  args = ap.parse_args()
  if args.combine:
    return combine(args.combine, args.out, args.baseline_name, args.bench_py)
  if not torch.cuda.is_available():
    sys.exit('bench_stream_hotwords.py needs a GPU')
  dev = torch.device('cuda:0')
  text, words = synthetic_arpa(1234, args.unigrams, args.bigrams, args.trigrams)
  spelled = spelled_logits(77, words[:5000], B0, T)
  if args.existing:
    L, h = baseline_library(args.existing, text.encode(), None)
    for name in STREAM + ('st_ctc_beam_ws',):
      getattr(L, name).restype, getattr(L, name).argtypes = _lib._SIGNATURES[name]
    samples = measure_existing(L, h, spelled, args.streams, args.rounds, dev)
    with open(args.out, 'w') as f:
      json.dump(dict(label=args.label, library=os.path.abspath(args.existing), samples=samples), f)
    print(json.dumps({k: round(float(np.median(v)), 4) for k, v in samples.items()}))
    return
  with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, 'synthetic.arpa')
    with open(path, 'w') as f:
      f.write(text)
    lm = LanguageModel(path)
  del text
  lib = _lib.load()
  handle = lm.device_handle(dev)
  rec = {'source_digest': source_digest(), 'device': torch.cuda.get_device_name(0), 'model': dict(lm.info, synthetic_seed=1234),
         'workload': 'the configs[4] shard\'s spelled logits as streams, {} rows per stream and step (200 ms), {} clocked steps after the '
                     'reset step, input log10(softmax + 1e-8); phrases of 5-15 characters drawn from the vocabulary the logits spell, '
                     'weight {}'.format(PER, STEPS, args.weight),
         'method': 'HIP events around {} back-to-back calls (log-softmax rows + search kernel) on resident rows and tables; the '
                   'variants alternate inside each of {} rounds; median (min, max) of the rounds'.format(STEPS, args.rounds)}

  # the phrase sets, each as the one real set of a HotwordSets (set 0, the empty one, in front): every stream starts at its root
  bias = {}
  for count in (100, 1000):
    sets = HotwordSets([Hotwords(phrases_from(words, count, count), args.weight)])
    tabs = sets.device_tables(dev)
    struct = _lib.BiasTables(tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), sets.n_states)
    bias[count] = (sets, tabs, struct)
  torch.cuda.synchronize()

  # ---- (b), (c) ------------------------------------------------------------------------------------------------------------
  biased = []
  for S in args.streams:
    x = Inputs(S, spelled, dev)
    for kind, beam, h in (('lm_free_beam16', 16, None), ('lm_beam100', 100, handle)):
      roots = {c: torch.full((S,), b[0].root(1), dtype=torch.int32, device=dev) for c, b in bias.items()}
      runs = {'unbiased': (Steps(lib, x, beam, h, dev), 'step')}
      for c, b in bias.items():
        runs['hot{}'.format(c)] = (Steps(lib, x, beam, h, dev, (b[1], b[2], roots[c])), 'step')
      us = {k: [] for k in runs}
      for _ in range(args.rounds):
        for k, (st, how) in runs.items():
          us[k].append(st.run(how))
      med = {k: float(np.median(v)) for k, v in us.items()}
      r = dict(kind=kind, beam=beam, streams=S, rows_per_step=PER, us_per_frame={k: spread(v) for k, v in us.items()},
               us_per_200ms_step={k: round(med[k] * PER, 2) for k in med},
               record_bytes=dict(unbiased=runs['unbiased'][0].state_bytes, biased=runs['hot100'][0].state_bytes))
      for c in bias:
        k = 'hot{}'.format(c)
        r['biased_over_unbiased_' + k] = dict(median=round(med[k] / med['unbiased'], 4),
                                               rounds=spread([p / q for p, q in zip(us[k], us['unbiased'])]))
      # (c) the read-outs of the open streams after the clocked steps, with what they walk: the labels that are not final yet
      read_us, tails = {}, {}
      for k in ('unbiased', 'hot1000'):
        st = runs[k][0]
        read_us[k] = [events(st.read, 50) * 1e3 for _ in range(args.rounds)]
        info = st.result.cpu().numpy().reshape(-1, 4)[:S]
        assert (info[:, 3] == 0).all(), info
        tails[k] = dict(hypothesis_len=int(np.median(info[:, 0])), unstable_tail=int(np.median(info[:, 0] - info[:, 1])))
      r['read_us'] = {k: spread(v) for k, v in read_us.items()}
      r['read_walks'] = tails
      biased.append(r)
      print(json.dumps(r), flush=True)
      del runs
    del x
    torch.cuda.empty_cache()
  rec['biased_stream'] = biased
  rec['tables'] = {str(c): dict(states=b[0].n_states, table_bytes=int(b[0].next.nbytes + b[0].gain.nbytes + b[0].fin.nbytes))
                   for c, b in bias.items()}
  yard = os.path.join(ROOT, 'profiles', 'hotwords.json')
  if os.path.exists(yard):
    with open(yard) as f:
      rec['offline_yardstick_biased_over_unbiased'] = json.load(f).get('biased_over_unbiased_nbest1')
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(rec, f, indent=1)
    f.write('\n')


if __name__ == '__main__':
  main()
