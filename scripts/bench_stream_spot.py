#!/usr/bin/env python3
"""Keyword spotting in live streams (StreamingRecognizer(spot=...), st_ctc_spot_stream_step): what it costs.

  --part kernel    st_ctc_spot_stream_step alone, 10 rows per stream and step, 64 streams, 1 / 16 / 256 keywords of 3-12 ids, packed
                   and with one keyword per wave, in steady state (no reset, the state carried), beside st_ctc_spot_f32 on the same
                   rows as one batch of 10-frame utterances and on 64 x 501 frames x 256 keywords (the shape of profiles/spot.json)
                   in the same session: time per (lattice, frame) and the ratios.  HIP events, median of 5 x 20 calls.
  --part step      a 200 ms step of the full-size 80-mel model with and without a spotter, alternating in one process, at 1 / 16 /
                   64 streams and 1 / 16 / 256 keywords; greedy, and (unless --no-lm) beam 100 with the synthetic trigram of
                   scripts/bench_lm_decode.py.  Host clock around 20 steps that end in a device synchronise.  The model's weights
                   are random and its posteriors nearly flat, so at the default threshold nearly every reading is a hit and the
                   step pays for thousands of `Hit` objects (hits_per_step); --threshold 0 --key whole_step_80mel_quiet measures
                   the machinery with hits as rare as they are in use.
  --part existing  the paths that run no new code -- the plain greedy step (16 streams), st_ctc_spot_f32 at 64 x 501 x 256 -- for
                   runs that alternate between this tree and the parent commit's (the caller alternates the processes and hands
                   the lines to --part merge).
  --part merge     fold the JSON lines of such runs (--lines FILE, each line tagged by --tag) into the output.

Writes / updates profiles/stream_spot.json (--output)."""
import argparse, ctypes, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from speecht_amd import _lib  # noqa: E402
from speecht_amd._lib import Tensor3  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--part', choices=['kernel', 'step', 'existing', 'merge'], required=True)
ap.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'stream_spot.json'))
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--no-lm', action='store_true')
ap.add_argument('--tag', default='this')
ap.add_argument('--lines', default=None)
ap.add_argument('--bench-lines', default=None, help='merge: lines "<tag> <the JSON line of bench.py>"')
ap.add_argument('--threshold', type=float, default=-0.69, help='step: the spotter\'s threshold (0: only exact readings are hits)')
ap.add_argument('--key', default='whole_step_80mel', help='step: the key of the output the shapes go to')
a = ap.parse_args()
C, DEV, ROWS = 29, 'cuda:0', 10


def update(key, value):
  out = {}
  if os.path.exists(a.output):
    with open(a.output) as f:
      out = json.load(f)
  out[key] = value
  os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
  with open(a.output, 'w') as f:
    json.dump(out, f, indent=1)
    f.write('\n')


def spread(v):
  return dict(median=round(sorted(v)[len(v) // 2], 5), min=round(min(v), 5), max=round(max(v), 5))


if a.part == 'merge':
  rows = [json.loads(l) for l in open(a.lines) if l.startswith('{')]
  for l in open(a.bench_lines) if a.bench_lines else ():
    tag, _, line = l.partition(' ')
    rows.append(dict(tag=tag, bench_py_utterances_per_s=json.loads(line)['value']))
  merged = {}
  for r in rows:
    for k, v in r.items():
      if k != 'tag':
        merged.setdefault(k, {}).setdefault(r['tag'], []).append(v)
  res = {k: {tag: dict(spread(v), runs=v) for tag, v in tags.items()} for k, tags in merged.items()}
  for k, tags in res.items():
    if 'this' in tags and 'parent' in tags:
      tags['this_median_inside_parent_spread'] = bool(tags['parent']['min'] <= tags['this']['median'] <= tags['parent']['max'])
  update('existing_paths_alternating_processes', res)
  print(json.dumps(res))
  sys.exit(0)

if not torch.cuda.is_available():
  sys.exit('bench_stream_spot.py needs a GPU')
lib = _lib.load()
P = lambda t: ctypes.c_void_p(t.data_ptr())
H = lambda x: ctypes.c_void_p(x.ctypes.data)
STREAM = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
to = lambda v: torch.as_tensor(np.ascontiguousarray(v)).to(DEV)


def median_us(fn, rounds=5, calls=20):
  for _ in range(3):
    fn()
  torch.cuda.synchronize()
  times = []
  for _ in range(rounds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
      fn()
    e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1) / calls * 1e3)
  return sorted(times)[rounds // 2], [round(t, 1) for t in times]


def csr(lists):
  offs = np.zeros(len(lists) + 1, dtype=np.int32)
  offs[1:] = np.cumsum([len(l) for l in lists])
  return np.array([i for l in lists for i in l] + [0], dtype=np.int32), offs


def keywords_of(K, rng):
  return [rng.integers(0, C - 1, size=int(rng.integers(3, 13))).tolist() for _ in range(K)]


def offline(B, T, keywords, logits):
  """st_ctc_spot_f32 on logits [B, T, C], every (utterance, keyword) pair -> a function that enqueues one call."""
  K, max_len = len(keywords), max(len(k) for k in keywords)
  ids, offs = csr(keywords)
  jobs = np.array([(b, k) for b in range(B) for k in range(K)], dtype=np.int32)
  n = len(jobs)
  x = torch.zeros((B, T, 32), dtype=torch.float32, device=DEV)
  x[:, :, :C] = torch.as_tensor(logits)
  desc = Tensor3(x.data_ptr(), B, T, C, 0, T, 32)
  keep = [x, to(ids), to(offs), to(np.full(B, T, dtype=np.int32)), to(jobs.reshape(-1)), torch.empty(n, dtype=torch.float64, device=DEV),
          torch.empty((n, 2), dtype=torch.int32, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)]
  need = lib.st_ctc_spot_ws(B, T, max_len, n)
  ws = torch.empty(need // 4 + 4, dtype=torch.int32, device=DEV)
  return lambda: _lib.call('st_ctc_spot_f32', ctypes.byref(desc), P(keep[3]), P(keep[1]), P(keep[2]), K, max_len, P(keep[4]), n, P(keep[5]),
                           P(keep[6]), None, None, P(keep[7]), P(ws), need, STREAM)


def big_offline():
  rng = np.random.default_rng(0)
  logits = rng.normal(size=(64, 501, C)).astype(np.float32)
  return offline(64, 501, keywords_of(256, rng), logits)


if a.part == 'kernel':
  S, res = 64, []
  big_us, big_all = median_us(big_offline())
  big_ns = big_us * 1e3 / (64 * 256 * 501)
  for K in (1, 16, 256):
    rng = np.random.default_rng(K)
    keywords = keywords_of(K, rng)
    logits = rng.normal(size=(S, ROWS, C)).astype(np.float32)
    ids, offs = csr(keywords)
    r = dict(streams=S, keywords=K, rows_per_stream=ROWS)
    for pack in (1, 0):
      size = int(lib.st_ctc_spot_stream_plan_bytes(H(ids), H(offs), K, C, pack))
      plan, waves = np.zeros(size // 4, dtype=np.int32), ctypes.c_int(0)
      _lib.call('st_ctc_spot_stream_plan', H(ids), H(offs), K, C, pack, H(plan), ctypes.byref(waves))
      d_plan = to(plan)
      _lib.call('st_ctc_spot_stream_plan_bind', H(plan), P(d_plan))
      state = torch.zeros(S * int(lib.st_ctc_spot_stream_state_bytes(H(plan))) // 8, dtype=torch.int64, device=DEV)
      x = torch.zeros((S * ROWS, 32), dtype=torch.float32, device=DEV)
      x[:, :C] = torch.as_tensor(logits.reshape(-1, C))
      rows = to(np.array([(s, 100 + i) for s in range(S) for i in range(ROWS)], dtype=np.int32))
      table = lambda reset: to(np.array([(s * ROWS, ROWS, -1, reset) for s in range(S)], dtype=np.int32))
      first, steady = table(1), table(0)
      events = torch.zeros(S * 64 * 8, dtype=torch.int32, device=DEV)
      counts = torch.zeros(S, dtype=torch.int32, device=DEV)
      run = lambda t: _lib.call('st_ctc_spot_stream_step', P(x), 32, C, P(rows), P(t), S * ROWS, S, H(plan), -0.69, 15, P(state), P(events), 64,
                                P(counts), STREAM)
      run(first)
      us, us_all = median_us(lambda: run(steady))
      tag = 'packed' if pack else 'one_keyword_per_wave'
      r[tag] = dict(waves_per_stream=waves.value, states_per_lane=int(plan[4]), us=round(us, 2), us_all=us_all,
                    ns_per_lattice_frame=round(us * 1e3 / (S * K * ROWS), 4), state_bytes_per_stream=int(state.numel() * 8 // S))
    off_us, off_all = median_us(offline(S, ROWS, keywords, logits))
    r['offline_same_rows'] = dict(us=round(off_us, 2), us_all=off_all, ns_per_lattice_frame=round(off_us * 1e3 / (S * K * ROWS), 4))
    r['packed_over_one_keyword_per_wave'] = round(r['packed']['us'] / r['one_keyword_per_wave']['us'], 4)
    r['packed_over_offline_same_rows'] = round(r['packed']['us'] / off_us, 4)
    r['packed_ns_over_offline_64x501x256_ns'] = round(r['packed']['ns_per_lattice_frame'] / big_ns, 2)
    print(json.dumps(r), flush=True)
    res.append(r)
  update('kernel', dict(device=torch.cuda.get_device_name(0), method='HIP events around 20 back-to-back calls, median of 5 rounds; the stream '
                        'step is a memset of the counts and one launch, the offline call two launches', threshold=-0.69, hold_frames=15,
                        offline_64x501x256=dict(us=round(big_us, 1), us_all=big_all, ns_per_lattice_frame=round(big_ns, 4)), shapes=res))
  sys.exit(0)

from speecht_amd.engine import Wav2LetterEngine  # noqa: E402
from speecht_amd.streaming import StreamBeam, StreamingRecognizer  # noqa: E402
from tests.workloads import synthetic_features, w2l_layers  # noqa: E402
NEW = 20                       # input frames per step: 200 ms


def clock(fn, calls):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(calls):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / calls * 1e3


seen, steps = [0], [0]           # hits (the lost ones included) and steps of the recogniser with a spotter being timed


def stepper(rec, S, x):
  slots = [rec.open() for _ in range(S)]
  at = [0]

  def step():
    if at[0] + NEW > x.shape[1]:
      at[0] = 0
    r = rec.step({slots[s]: x[s, at[0]:at[0] + NEW] for s in range(S)})
    at[0] += NEW
    if rec.spot is not None:
      steps[0] += 1
      seen[0] += sum(len(v) for v in r.hits.values()) + sum(r.hits_lost.values())

  for _ in range(8):
    step()
  return step


eng = Wav2LetterEngine(w2l_layers(80), device=DEV)
eng.init_xavier(42)

if a.part == 'existing':
  S = 16
  x = np.stack([synthetic_features(s, 4000, 80) for s in range(S)]).astype(np.float32)
  step = stepper(StreamingRecognizer(eng, S, max_chunk_frames=NEW), S, x)
  plain = sorted(clock(step, 20) for _ in range(a.rounds))[a.rounds // 2]
  spot_us, _ = median_us(big_offline())
  print(json.dumps(dict(tag=a.tag, plain_greedy_step_ms_16_streams=round(plain, 5), offline_spot_us_64x501x256=round(spot_us, 1))), flush=True)
  sys.exit(0)

from speecht_amd.streaming import StreamSpotter  # noqa: E402
from speecht_amd import vocabulary  # noqa: E402
lm = None
if not a.no_lm:
  import tempfile
  import bench_lm_decode as BL  # noqa: E402
  from speecht_amd.language_model import LanguageModel  # noqa: E402
  text, _ = BL.synthetic_arpa(1234, 200000, 1000000, 1000000)
  with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, 'synthetic.arpa')
    with open(path, 'w') as f:
      f.write(text)
    lm = LanguageModel(path)
  del text
res = []
for S in (1, 16, 64):
  x = np.stack([synthetic_features(s, 4000, 80) for s in range(S)]).astype(np.float32)
  beams = {'greedy': lambda: None}
  if lm is not None:
    beams['beam100_lm'] = lambda: StreamBeam(lm=lm, max_seconds=120.0, max_tail=2048)
  for K in (1, 16, 256):
    rng = np.random.default_rng(K)
    texts = sorted({vocabulary.ids_to_sentence(k) for k in keywords_of(2 * K, rng)})[:K]
    r = dict(streams=S, keywords=len(texts), new_frames_per_step=NEW)
    for name, make in beams.items():
      forms = {'plain': stepper(StreamingRecognizer(eng, S, max_chunk_frames=NEW, beam=make()), S, x)}
      rec = StreamingRecognizer(eng, S, max_chunk_frames=NEW, beam=make(), spot=StreamSpotter(texts, threshold=a.threshold))
      seen[0], steps[0] = 0, 0
      forms['spot'] = stepper(rec, S, x)
      t = {k: [] for k in forms}
      for _ in range(a.rounds):
        for k, fn in forms.items():
          t[k].append(clock(fn, 20))
      r[name] = dict(hits_per_step=round(seen[0] / float(steps[0]), 2), plain_step_ms=spread(t['plain']), spot_step_ms=spread(t['spot']),
                     ratio_spot_over_plain=spread([p / q for p, q in zip(t['spot'], t['plain'])]), waves_per_stream=rec.spot_waves)
      del forms, rec
      torch.cuda.empty_cache()
    print(json.dumps(r), flush=True)
    res.append(r)
update(a.key, dict(device=torch.cuda.get_device_name(0), rounds=a.rounds,
                                timing='host clock around 20 steps that end in a device synchronise; the forms alternate inside every round',
                                threshold=a.threshold, hold_seconds=0.3, shapes=res))
