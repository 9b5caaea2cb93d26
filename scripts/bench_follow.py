#!/usr/bin/env python3
"""Following a known script in live streams (StreamingRecognizer(follow=...), st_ctc_follow_stream_step): what it costs.

  --part kernel    st_ctc_follow_stream_step alone in steady state (no reset, the state carried, so many frames in that no block is
                   skipped): 64 rows per stream and step, 1 and 16 streams, scripts of 500 and 9 000 labels (2 and 21 state blocks);
                   time per run of 64 rows (softmax, tile and read-out launches) and per (state block, frame), beside
                   st_ctc_align_long_f32's time per frame-block launch (the figure of scripts/bench_align_long.py: the whole call
                   over its launches) at 9 000 labels x 16 384 frames in the same session.  One stream is the like-for-like shape:
                   both then launch 21 waves per 64 frames.  The frame loops differ in the per-frame wave reduction that stands in
                   the place of the back-pointer store.  HIP events, median of 5 x 20 calls.
  --part step      a 200 ms step of the full-size 80-mel model with and without a follower, alternating in one process, at 1 / 16 /
                   64 streams and scripts of 500 and 9 000 labels; greedy, and (unless --no-lm) beam 100 with the synthetic trigram
                   of scripts/bench_lm_decode.py.  Host clock around 20 steps that end in a device synchronise.
  --part existing  the paths that run no new code -- the plain greedy step (16 streams), the step with a spotter,
                   st_ctc_align_long_f32 -- for runs that alternate between this tree and the parent commit's (the caller
                   alternates the processes and hands the lines to --part merge).
  --part merge     fold the JSON lines of such runs (--lines FILE, each line tagged by --tag) into the output.

Writes / updates profiles/follow.json (--output)."""
import argparse, ctypes, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from speecht_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--part', choices=['kernel', 'step', 'existing', 'merge'], required=True)
ap.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'follow.json'))
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--no-lm', action='store_true')
ap.add_argument('--streams', default='1,16,64', help='step: the stream counts')
ap.add_argument('--tag', default='this')
ap.add_argument('--lines', default=None)
ap.add_argument('--bench-lines', default=None, help='merge: lines "<tag> <the JSON line of bench.py>"')
a = ap.parse_args()
C, DEV = 29, 'cuda:0'


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
  sys.exit('bench_follow.py needs a GPU')
lib = _lib.load()
P = lambda t: ctypes.c_void_p(t.data_ptr())
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


def align_long_call(T, L, rng):
  """st_ctc_align_long_f32 on T random rows and L labels -> a function that enqueues one call."""
  x = torch.zeros((T, 32), dtype=torch.float32, device=DEV)
  x[:, :C] = torch.as_tensor(rng.normal(size=(T, C)).astype(np.float32))
  ids = to(((np.arange(L) * 5) % (C - 1)).astype(np.int32))          # no adjacent repeats: the label fits T >= L frames
  assert T >= L
  spans = torch.empty((L, 2), dtype=torch.int32, device=DEV)
  score, status = torch.empty(1, dtype=torch.float64, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV)
  need = int(lib.st_ctc_align_long_ws(T, L))
  ws = torch.empty(need // 8 + 2, dtype=torch.float64, device=DEV)
  keep = [x, ids, spans, score, status, ws]
  return lambda: (keep, _lib.call('st_ctc_align_long_f32', P(x), T, C, 32, P(ids), L, P(spans), P(score), P(status), P(ws), need, STREAM))[1]


if a.part == 'kernel':
  ROWS, res = 64, []
  rng = np.random.default_rng(0)
  T_AL, L_AL = 16384, 9000
  call = align_long_call(T_AL, L_AL, rng)
  al_us, al_all = median_us(call, calls=3)
  nb_al, launches = (2 * L_AL + 1 + 895) // 896, T_AL // 64 + 3
  al = dict(frames=T_AL, labels=L_AL, state_blocks=nb_al, launches=launches, whole_call_us=round(al_us, 1), whole_call_us_all=al_all,
            us_per_frame_block_launch=round(al_us / launches, 2), ns_per_block_frame=round(al_us * 1e3 / (nb_al * T_AL), 3))
  print(json.dumps(al), flush=True)
  for S, L in ((1, 500), (1, 9000), (16, 500), (16, 9000)):
    nb = (2 * L + 1 + 895) // 896
    scripts = [rng.integers(0, C - 1, size=L).astype(np.int32) for _ in range(S)]
    ids, offs = to(np.concatenate(scripts)), to(np.arange(S + 1, dtype=np.int32) * L)
    starts, woffs = to(np.zeros(S, dtype=np.int32)), to(np.arange(S + 1, dtype=np.int32))
    x = torch.zeros((S * ROWS, 32), dtype=torch.float32, device=DEV)
    x[:, :C] = torch.as_tensor(rng.normal(size=(S * ROWS, C)).astype(np.float32))
    state = torch.zeros(S * int(lib.st_ctc_follow_stream_state_bytes(L)) // 8, dtype=torch.float64, device=DEV)
    need = int(lib.st_ctc_follow_stream_ws(S * ROWS, L, S))
    ws = torch.empty(need // 8 + 2, dtype=torch.float64, device=DEV)
    events, result = torch.zeros(S * 64 * 2, dtype=torch.int32, device=DEV), torch.zeros(S * 16, dtype=torch.int32, device=DEV)
    rows = to(np.array([(s, i) for s in range(S) for i in range(ROWS)], dtype=np.int32))
    table = lambda reset: to(np.array([(s * ROWS, ROWS, -1, reset) for s in range(S)], dtype=np.int32))
    first, steady = table(1), table(0)
    run = lambda t: _lib.call('st_ctc_follow_stream_step', P(x), 32, C, P(rows), P(t), S * ROWS, S * ROWS, ROWS, S, P(ids), P(offs), P(starts),
                              P(woffs), L, 3, P(state), P(events), 64, P(result), None, P(ws), need, STREAM)
    run(first)
    for _ in range(-(-L // ROWS)):                                 # until 2 t + 1 has passed the last block: no tile is skipped
      run(steady)
    us, us_all = median_us(lambda: run(steady))
    r = dict(streams=S, labels=L, state_blocks=nb, rows_per_stream=ROWS, us_per_run=round(us, 2), us_all=us_all,
             ns_per_block_frame=round(us * 1e3 / (S * nb * ROWS), 3), state_bytes_per_stream=int(state.numel() * 8 // S))
    r['run_over_align_long_frame_block_launch'] = round(us / al['us_per_frame_block_launch'], 3)
    r['per_block_frame_over_align_long'] = round(r['ns_per_block_frame'] / al['ns_per_block_frame'], 3)
    print(json.dumps(r), flush=True)
    res.append(r)
  update('kernel', dict(device=torch.cuda.get_device_name(0), method='HIP events around 20 back-to-back steps (softmax, tile and read-out '
                        'launches), median of 5 rounds; align_long: the whole call over its launches (3 calls per round)', confirm_frames=3, align_long=al, shapes=res))
  sys.exit(0)

from speecht_amd.engine import Wav2LetterEngine  # noqa: E402
from speecht_amd.streaming import StreamBeam, StreamingRecognizer, StreamSpotter  # noqa: E402
from tests.workloads import synthetic_features, w2l_layers  # noqa: E402
NEW = 20                       # input frames per step: 200 ms


def clock(fn, calls):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(calls):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / calls * 1e3


def stepper(rec, S, x, script=None):
  slots = [rec.open(script=script) if script is not None else rec.open() for _ in range(S)]
  at = [0]

  def step():
    if at[0] + NEW > x.shape[1]:
      at[0] = 0
    rec.step({slots[s]: x[s, at[0]:at[0] + NEW] for s in range(S)})
    at[0] += NEW

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
  step = stepper(StreamingRecognizer(eng, S, max_chunk_frames=NEW, spot=StreamSpotter(['hello', 'the cat', 'world'], threshold=0.0)), S, x)
  spot = sorted(clock(step, 20) for _ in range(a.rounds))[a.rounds // 2]
  al_us, _ = median_us(align_long_call(4096, 4000, np.random.default_rng(0)), calls=5)
  print(json.dumps(dict(tag=a.tag, plain_greedy_step_ms_16_streams=round(plain, 5), spotter_step_ms_16_streams=round(spot, 5),
                        align_long_us_4096x4000=round(al_us, 1))), flush=True)
  sys.exit(0)

from speecht_amd.streaming import ScriptFollower  # noqa: E402
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
for S in [int(v) for v in a.streams.split(',')]:
  x = np.stack([synthetic_features(s, 4000, 80) for s in range(S)]).astype(np.float32)
  beams = {'greedy': lambda: None}
  if lm is not None:
    beams['beam100_lm'] = lambda: StreamBeam(lm=lm, max_seconds=120.0, max_tail=2048)
  for L in (500, 9000):
    rng = np.random.default_rng(L)
    script = rng.integers(0, C - 1, size=L).tolist()
    r = dict(streams=S, labels=L, state_blocks=(2 * L + 1 + 895) // 896, new_frames_per_step=NEW)
    for name, make in beams.items():
      forms = {'plain': stepper(StreamingRecognizer(eng, S, max_chunk_frames=NEW, beam=make()), S, x)}
      rec = StreamingRecognizer(eng, S, max_chunk_frames=NEW, beam=make(), follow=ScriptFollower(max_labels=L))
      forms['follow'] = stepper(rec, S, x, script)
      t = {k: [] for k in forms}
      for _ in range(a.rounds):
        for k, fn in forms.items():
          t[k].append(clock(fn, 20))
      r[name] = dict(plain_step_ms=spread(t['plain']), follow_step_ms=spread(t['follow']),
                     ratio_follow_over_plain=spread([p / q for p, q in zip(t['follow'], t['plain'])]))
      del forms, rec
      torch.cuda.empty_cache()
    print(json.dumps(r), flush=True)
    res.append(r)
update('whole_step_80mel', dict(device=torch.cuda.get_device_name(0), rounds=a.rounds,
                                timing='host clock around 20 steps that end in a device synchronise; the forms alternate inside every round',
                                confirm_seconds=0.06, shapes=res))
