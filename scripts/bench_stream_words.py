#!/usr/bin/env python3
"""Word times and confidences for the finals of live streams (StreamingRecognizer(words=FinalWords(...)), st_stream_keep_f32,
st_ctc_align_ring_f32, st_ctc_word_conf_ring_f32): what they cost.

By the protocol of scripts/bench_endpoint.py: the full-size 80-mel model, 200 ms of audio per stream and step, 1 / 16 / 64 streams,
greedy and beam 100 with the synthetic 200 k / 1 M / 1 M trigram of scripts/bench_lm_decode.py; the forms alternate inside every round.

  (a) quiet    an endpointed step with words against one without, no event firing: the difference is the keep launch;
  (b) events   the same with an endpoint every 3 s of every stream: the extra time per final (upload, six launches, a second wait);
  (c) lattices st_ctc_align_ring_f32 / st_ctc_word_conf_ring_f32 alone on 64 jobs of 150 rows x 30-45 labels against st_ctc_align_f32 /
               st_ctc_word_conf_f32 on the same rows in a dense tensor: only the first stage's addressing differs;
  (d) existing with --parent DIR (a built tree of the commit before): the plain step, the endpointed step without words,
               st_ctc_align_f32, st_ctc_word_conf_f32 and bench.py in alternating processes, this tree against that one, each ratio beside
               the parent's own max / min over its repeats.

Writes profiles/stream_words.json (--output)."""
import argparse, ctypes, json, os, subprocess, sys, tempfile, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'stream_words.json'))
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--streams', type=int, nargs='+', default=[1, 16, 64])
ap.add_argument('--unigrams', type=int, default=200000)
ap.add_argument('--bigrams', type=int, default=1000000)
ap.add_argument('--trigrams', type=int, default=1000000)
ap.add_argument('--parent', default=None, help='a built tree of the parent commit: also measure (d)')
ap.add_argument('--repeats', type=int, default=3, help='(d): processes per tree')
ap.add_argument('--bench-steps', type=int, default=20)
ap.add_argument('--skip', nargs='*', default=[], help='parts to leave out: steps lattices')
ap.add_argument('--existing-child', default=None, metavar='TREE', help='(internal) measure the existing paths of TREE, print one JSON line')
a = ap.parse_args()
TREE = os.path.abspath(a.existing_child) if a.existing_child else ROOT
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(TREE, 'scripts'))
import torch  # noqa: E402
from speecht_amd import _lib  # noqa: E402
from speecht_amd.engine import Wav2LetterEngine  # noqa: E402
from speecht_amd.streaming import Endpointing, StreamBeam, StreamingRecognizer  # noqa: E402
from tests.workloads import synthetic_features, w2l_layers  # noqa: E402

if not torch.cuda.is_available():
  sys.exit('bench_stream_words.py needs a GPU')
NEW = 20                       # input frames per step: 200 ms


def clock(fn, calls):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(calls):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / calls * 1e3


def spread(v):
  return dict(median=round(sorted(v)[len(v) // 2], 5), min=round(min(v), 5), max=round(max(v), 5))


def speech_engine():
  eng = Wav2LetterEngine(w2l_layers(80), device='cuda:0')
  eng.init_xavier(42)
  weights = [(np.asarray(F), np.array(b)) for F, b in eng.get_weights()]
  weights[-1][1][-1] -= 1000.0                                    # the blank never wins: every row is speech
  eng.set_weights(weights)
  return eng


def stepper(rec, x, S, count_finals):
  slots = [rec.open() for _ in range(S)]
  at, seen = [0], [0]

  def step():
    if at[0] + NEW > x.shape[1]:
      at[0] = 0
    r = rec.step({slots[s]: x[s, at[0]:at[0] + NEW] for s in range(S)})
    at[0] += NEW
    if count_finals:
      seen[0] += sum(len(v) for v in r.finals.values())

  for _ in range(8):
    step()
  return step, seen


def lattice_case(dev, jobs=64, rows=150, C=29, space=27, seed=7, with_ring=True):
  """(c): the same utterances in a ring (frames 100 .. 249 of 64 streams, cap 160: they wrap) and in a dense tensor.
  ``with_ring=False``: the dense entry points alone (a tree of the parent commit has no others)."""
  lib = _lib.load()
  rng = np.random.default_rng(seed)
  x = (rng.standard_normal((jobs, rows, C)) * 2.0).astype(np.float32)
  labels = []
  for j in range(jobs):
    lab = [int(v) for v in rng.integers(0, 26, int(rng.integers(30, 46)))]
    for i in range(5, len(lab), 6):
      lab[i] = space
    for i in range(1, len(lab)):
      if lab[i] == lab[i - 1]:
        lab[i] = (lab[i] + 1) % 26
    labels.append(lab)
  from speecht_amd.alignment import word_runs
  runs = [word_runs(l, space) for l in labels]
  offs = np.zeros(jobs + 1, np.int32)
  offs[1:] = np.cumsum([len(l) for l in labels])
  N, W, max_len = int(offs[-1]), sum(len(r) for r in runs), max(len(l) for l in labels)
  to = lambda arr, dt=np.int32: torch.from_numpy(np.ascontiguousarray(arr, dtype=dt)).to(dev)
  p = lambda t: ctypes.c_void_p(t.data_ptr())
  d_ids, d_offs = to([i for l in labels for i in l] + [0]), to(offs)
  d_wspans = to([(j, s, e) for j, r in enumerate(runs) for s, e in r])
  cap, u0 = rows + 10, 100                                        # st_stream_keep_rows(rows, 10)
  ring = torch.zeros(jobs * cap * 32, dtype=torch.float32, device=dev)
  dense = torch.zeros(jobs, rows, 32, dtype=torch.float32, device=dev)
  dense[:, :, :C] = to(x, np.float32)
  table = to([(j, u0 + t) for j in range(jobs) for t in range(rows)])
  if with_ring:
    _lib.call('st_stream_keep_f32', p(dense), 32, C, p(table), jobs * rows, jobs, p(ring), cap, None)
  d_jobs, d_lens = to([(j, u0, rows) for j in range(jobs)]), to([rows] * jobs)
  t3 = _lib.Tensor3(dense.data_ptr(), jobs, rows, C, 0, rows, 32)
  need_a, need_c = int(lib.st_ctc_align_ws(jobs, rows, max_len)), int(lib.st_ctc_word_conf_ws(jobs, rows, max_len, jobs + W))
  ws = torch.empty(max(need_a, need_c) // 4 + 4, dtype=torch.int32, device=dev)
  out = {k: (torch.zeros(2 * N, dtype=torch.int32, device=dev), torch.zeros(jobs, dtype=torch.float32, device=dev),
             torch.zeros(jobs, dtype=torch.int32, device=dev), torch.zeros(jobs, dtype=torch.float64, device=dev),
             torch.zeros(W, dtype=torch.float64, device=dev)) for k in ('ring', 'dense')}
  fns = {
      'align_ring': lambda: _lib.call('st_ctc_align_ring_f32', p(ring), jobs, cap, C, p(d_jobs), jobs, rows, p(d_ids), p(d_offs), max_len,
                                      p(out['ring'][0]), None, p(out['ring'][1]), p(out['ring'][2]), p(ws), need_a, None),
      'align_dense': lambda: _lib.call('st_ctc_align_f32', ctypes.byref(t3), p(d_ids), p(d_offs), p(d_lens), max_len, p(out['dense'][0]), None,
                                       p(out['dense'][1]), p(out['dense'][2]), p(ws), need_a, None),
      'conf_ring': lambda: _lib.call('st_ctc_word_conf_ring_f32', p(ring), jobs, cap, C, p(d_jobs), jobs, rows, p(d_ids), p(d_offs), max_len,
                                     space, p(d_wspans), W, p(out['ring'][3]), p(out['ring'][4]), p(out['ring'][2]), p(ws), need_c, None),
      'conf_dense': lambda: _lib.call('st_ctc_word_conf_f32', ctypes.byref(t3), p(d_ids), p(d_offs), p(d_lens), max_len, space, p(d_wspans), W,
                                      p(out['dense'][3]), p(out['dense'][4]), p(out['dense'][2]), p(ws), need_c, None)}
  if not with_ring:
    fns = {k: fn for k, fn in fns.items() if k.endswith('dense')}
  for fn in fns.values():
    fn()
  torch.cuda.synchronize()
  same = with_ring and all(bool((r.view(torch.int32) == d.view(torch.int32)).all()) for r, d in zip(out['ring'], out['dense']))
  return fns, dict(jobs=jobs, rows=rows, labels='30-45', words=W, ring_cap=cap, ring_equals_dense_bit_for_bit=same), (fns, ring, dense, ws, out, t3)


def existing_child():
  """(d), one process: the existing paths of the tree this process imports."""
  dev = torch.device('cuda:0')
  eng = speech_engine()
  S = 16
  x = np.stack([synthetic_features(s, 4000, 80) for s in range(S)]).astype(np.float32)
  res = {}
  for name, ep in (('plain_step_ms', None), ('endpoint_step_ms', Endpointing(silence=0.5, lead=1.0, max_utterance=3.0))):
    step, _ = stepper(StreamingRecognizer(eng, S, max_chunk_frames=NEW, endpoint=ep), x, S, ep is not None)
    res[name] = min(clock(step, 20) for _ in range(3))
  fns, _, keep = lattice_case(dev, with_ring=False)
  for name, key in (('align_f32_ms', 'align_dense'), ('word_conf_f32_ms', 'conf_dense')):
    clock(fns[key], 5)
    res[name] = min(clock(fns[key], 20) for _ in range(3))
  print('CHILD ' + json.dumps(res), flush=True)


if a.existing_child:
  existing_child()
  sys.exit(0)

from speecht_amd.streaming import FinalWords  # noqa: E402
dev = torch.device('cuda:0')
out = dict(device=torch.cuda.get_device_name(0), rounds=a.rounds,
           timing='host clock around 20 steps (or calls) that end in a device synchronise; the forms alternate inside every round')

if 'lattices' not in a.skip:
  fns, info, keep = lattice_case(dev)
  t = {k: [] for k in fns}
  for fn in fns.values():
    clock(fn, 5)
  for _ in range(a.rounds):
    for k, fn in fns.items():
      t[k].append(clock(fn, 20))
  info.update({k + '_ms': spread(v) for k, v in t.items()})
  info['ratio_align_ring_over_dense'] = spread([r / d for r, d in zip(t['align_ring'], t['align_dense'])])
  info['ratio_conf_ring_over_dense'] = spread([r / d for r, d in zip(t['conf_ring'], t['conf_dense'])])
  out['lattices_64_jobs'] = info
  print(json.dumps(info), flush=True)
  del fns, keep

if 'steps' not in a.skip:
  import bench_lm_decode as BL  # noqa: E402
  from speecht_amd.language_model import LanguageModel  # noqa: E402
  text, _ = BL.synthetic_arpa(1234, a.unigrams, a.bigrams, a.trigrams)
  with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, 'synthetic.arpa')
    with open(path, 'w') as f:
      f.write(text)
    lm = LanguageModel(path)
  del text
  out['model'] = dict(lm.info, synthetic_seed=1234)
  eng = speech_engine()
  CASES = {'quiet': Endpointing(silence=0.5, lead=1.0, max_utterance=120.0), 'events': Endpointing(silence=0.5, lead=1.0, max_utterance=3.0)}
  res = []
  for case, endpoint in CASES.items():
    for S in a.streams:
      x = np.stack([synthetic_features(s, 4000, 80) for s in range(S)]).astype(np.float32)
      beams = {'greedy': lambda: None, 'beam100_lm': lambda: StreamBeam(lm=lm, max_seconds=120.0, max_tail=2048)}
      recs, steps, finals = {}, {}, {}
      for name, make in beams.items():
        for form, words in (('endpoint', None), ('words', FinalWords(timestamps=True, confidence=True))):
          rec = StreamingRecognizer(eng, S, max_chunk_frames=NEW, beam=make(), endpoint=endpoint, words=words)
          steps[name, form], finals[name, form] = stepper(rec, x, S, True)
          recs[name, form] = rec
      t = {key: [] for key in steps}
      before = {key: finals[key][0] for key in steps}
      for _ in range(a.rounds):
        for key in steps:
          t[key].append(clock(steps[key], 20))
      r = dict(case=case, streams=S, new_frames_per_step=NEW, max_utterance=endpoint.max_utterance)
      for name in beams:
        n_finals = finals[name, 'words'][0] - before[name, 'words']
        extra_ms = (sum(t[name, 'words']) - sum(t[name, 'endpoint'])) * 20
        r[name] = dict(endpoint_step_ms=spread(t[name, 'endpoint']), words_step_ms=spread(t[name, 'words']),
                       ratio_words_over_endpoint=spread([p / q for p, q in zip(t[name, 'words'], t[name, 'endpoint'])]),
                       step_difference_us=round((sorted(t[name, 'words'])[a.rounds // 2] - sorted(t[name, 'endpoint'])[a.rounds // 2]) * 1e3, 2),
                       launches_last_pass=dict(endpoint=recs[name, 'endpoint'].launches, words=recs[name, 'words'].launches),
                       finals_in_timed_steps=n_finals,
                       extra_ms_per_final=round(extra_ms / n_finals, 5) if n_finals else None)
      print(json.dumps(r), flush=True)
      res.append(r)
      del recs, steps
      torch.cuda.empty_cache()
  out['whole_step_80mel'] = res

if a.parent:
  trees = {'this': ROOT, 'parent': os.path.abspath(a.parent)}
  runs = {k: [] for k in trees}
  for _ in range(a.repeats):                                       # alternating processes
    for k, tree in trees.items():
      p = subprocess.run([sys.executable, os.path.abspath(__file__), '--existing-child', tree], capture_output=True, text=True, timeout=600)
      line = [l for l in p.stdout.splitlines() if l.startswith('CHILD ')]
      if p.returncode != 0 or not line:
        sys.exit('the child on {} failed:\n{}\n{}'.format(tree, p.stdout[-2000:], p.stderr[-2000:]))
      r = json.loads(line[0][6:])
      b = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(a.bench_steps), '--warmup', '5'], cwd=tree,
                         capture_output=True, text=True, timeout=900)
      last = [l for l in b.stdout.splitlines() if l.startswith('{')]
      if b.returncode != 0 or not last:
        sys.exit('bench.py in {} failed:\n{}\n{}'.format(tree, b.stdout[-2000:], b.stderr[-2000:]))
      r['bench_py'] = json.loads(last[-1])
      runs[k].append(r)
      print(k, json.dumps(r), flush=True)
  keys = [k for k in runs['this'][0] if k != 'bench_py']
  cmp_ = {}
  for k in keys:
    mine, theirs = [r[k] for r in runs['this']], [r[k] for r in runs['parent']]
    cmp_[k] = dict(this=spread(mine), parent=spread(theirs), ratio_this_over_parent=round(sorted(mine)[len(mine) // 2] / sorted(theirs)[len(theirs) // 2], 4),
                   parent_max_over_min=round(max(theirs) / min(theirs), 4))
  mine, theirs = [r['bench_py']['value'] for r in runs['this']], [r['bench_py']['value'] for r in runs['parent']]
  cmp_['bench_py_utterances_per_s'] = dict(this=spread(mine), parent=spread(theirs), parent_max_over_min=round(max(theirs) / min(theirs), 4),
                                           ratio_this_over_parent=round(sorted(mine)[len(mine) // 2] / sorted(theirs)[len(theirs) // 2], 4))
  out['existing_paths_vs_parent'] = dict(streams=16, repeats=a.repeats, order='this tree first in every pair', paths=cmp_)

os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
with open(a.output, 'w') as f:
  json.dump(out, f, indent=1)
  f.write('\n')
