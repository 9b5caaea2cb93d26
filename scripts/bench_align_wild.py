#!/usr/bin/env python3
"""The wildcard entry points beside the plain ones, in one session, alternating round by round on the same logits:
  st_ctc_align_wild_f32 against st_ctc_align_f32 at the shapes of profiles/align.json
    64 x 501 output frames with 100-150 labels, 16 x 1 501 output frames with 300-450 labels (random logits),
  st_ctc_align_long_wild_f32 against st_ctc_align_long_f32 at the ten-minute shape of profiles/align_long.json
    41 400 output frames x 9 000 labels (planted logits),
29 classes.  Labels are text-like: words of 2-9 letters with the space id between them.  Each shape runs the plain entry point on
the labels as they are, and the wildcard entry point on the same labels (no wildcard: the same lattice), with every 20th word
replaced by one wildcard, and with a wildcard and a space added at both ends -- each with the fit stage off and on.  HIP events
around back-to-back calls; a round times every variant once, so a ratio is taken inside a round; reported: the median of the
rounds' ratios with their smallest and largest.  The fit stage's own time is the difference fit on - fit off of a round, at the
ten-minute shape once with ordinary spans and once with a single ordinary label forced over 5 000 frames, the serial worst case of
one lane per label.  Writes profiles/align_wild.json (--output)."""
import argparse, ctypes, json, os, subprocess, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'align_wild.json'))
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--parent', default=None, help='a built tree of the parent commit: also the existing paths of both trees, processes alternating')
ap.add_argument('--repeats', type=int, default=3, help='--parent: processes per tree')
ap.add_argument('--skip-new', action='store_true', help='--parent: only the existing paths')
ap.add_argument('--existing-child', default=None, metavar='TREE', help='(internal) measure the existing paths of TREE, print one JSON line')
a = ap.parse_args()
TREE = os.path.abspath(a.existing_child) if a.existing_child else ROOT
sys.path.insert(0, TREE)
from speecht_amd import _lib
from speecht_amd._lib import Tensor3
from tests import align_oracle as AO

C, PITCH, SPACE, W = 29, 32, 27, 29
BIAS = -1.0
DEV = 'cuda:0'
lib = _lib.load()
P = lambda t: ctypes.c_void_p(t.data_ptr())
to = lambda x: torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def text_labels(rng, L):
  """L ids: words of 2-9 letters (ids 0-26, some doubled letters) with one space between them."""
  out = []
  while len(out) < L:
    word = [int(c) for c in rng.integers(0, 27, int(rng.integers(2, 10)))]
    out += ([SPACE] if out else []) + word
  return out[:L - 1] + [int(rng.integers(0, 27))] if out[L - 1] == SPACE else out[:L]


def every_20th_word(lab):
  out, word, n = [], [], 0
  for i in lab + [SPACE]:
    if i != SPACE:
      word.append(i)
      continue
    if word:
      n += 1
      out += [W] if n % 20 == 0 else word
      word = []
    out.append(SPACE)
  return out[:-1]


def ends_only(lab):
  return [W, SPACE] + lab + [SPACE, W]


def alternating(variants, rounds, calls):
  """{name: fn} -> {name: [us per call in each round]}: every round times every variant once, in turn."""
  for fn in variants.values():
    fn()
  torch.cuda.synchronize()
  times = {k: [] for k in variants}
  for _ in range(rounds):
    for k, fn in variants.items():
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(calls):
        fn()
      e1.record()
      torch.cuda.synchronize()
      times[k].append(e0.elapsed_time(e1) / calls * 1e3)
  return times


def summary(times, base='plain'):
  med = lambda v: float(sorted(v)[len(v) // 2])
  out = {}
  for k, v in times.items():
    out[k] = dict(us=round(med(v), 1), us_min=round(min(v), 1), us_max=round(max(v), 1))
    if k != base:
      r = [x / y for x, y in zip(v, times[base])]
      out[k].update(over_plain=round(med(r), 4), over_plain_min=round(min(r), 4), over_plain_max=round(max(r), 4))
  return out


def fit_stage(times, name):
  d = [x - y for x, y in zip(times[name + ', fit'], times[name])]
  return dict(us=round(float(sorted(d)[len(d) // 2]), 1), us_min=round(min(d), 1), us_max=round(max(d), 1))


def batch_shape(rng, B, T, lo, hi, calls):
  labs = [text_labels(rng, int(rng.integers(lo, hi + 1))) for _ in range(B)]
  x = torch.zeros((B, T, PITCH), dtype=torch.float32, device=DEV)
  x[:, :, :C] = to(np.stack([AO.random_logits(rng, T, C, 1.0) for _ in range(B)]))
  desc = Tensor3(x.data_ptr(), B, T, C, 0, T, PITCH)
  d_lens = to(np.full(B, T, dtype=np.int32))
  stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
  keep, variants, status = [], {}, {}

  def variant(name, labels, wild, fit):
    lens = [len(l) for l in labels]
    offs = np.zeros(B + 1, dtype=np.int32)
    offs[1:] = np.cumsum(lens)
    N, max_len = int(offs[-1]), max(lens)
    d_ids, d_offs = to(np.array([i for l in labels for i in l] + [0], dtype=np.int32)), to(offs)
    spans = torch.empty((N, 2), dtype=torch.int32, device=DEV)
    states = torch.empty((B, T), dtype=torch.int32, device=DEV)
    score = torch.empty(B, dtype=torch.float32, device=DEV)
    stat = torch.empty(B, dtype=torch.int32, device=DEV)
    fits = torch.empty(N, dtype=torch.float64, device=DEV)
    need = lib.st_ctc_align_ws(B, T, max_len)
    ws = torch.empty(need // 4 + 4, dtype=torch.int32, device=DEV)
    keep.append((d_ids, d_offs, spans, states, score, stat, fits, ws))
    if wild:
      variants[name] = lambda: _lib.call('st_ctc_align_wild_f32', ctypes.byref(desc), P(d_ids), P(d_offs), P(d_lens), max_len, BIAS,
                                         P(spans), P(states), P(score), P(stat), P(fits) if fit else None, P(ws), need, stream)
    else:
      variants[name] = lambda: _lib.call('st_ctc_align_f32', ctypes.byref(desc), P(d_ids), P(d_offs), P(d_lens), max_len, P(spans),
                                         P(states), P(score), P(stat), P(ws), need, stream)
    status[name] = stat

  variant('plain', labs, False, False)
  for name, labels in (('no wildcard', labs), ('every 20th word', [every_20th_word(l) for l in labs]), ('ends only', [ends_only(l) for l in labs])):
    variant(name, labels, True, False)
    variant(name + ', fit', labels, True, True)
  times = alternating(variants, a.rounds, calls)
  assert all(int(s.abs().sum().cpu()) == 0 for s in status.values())
  return dict(batch=B, output_frames=T, label_lengths=[lo, hi], calls_per_round=calls, rounds=a.rounds, variants=summary(times))


def planted_text(rng, T, L, forced=0):
  """Planted logits of text-like labels; ``forced``: that many frames in the middle on which ONE further label is planted."""
  lab = text_labels(rng, L)
  if not forced:
    return AO.planted_logits(rng, lab, T, C)[0], lab, None
  half = L // 2
  while lab[half - 1] == 5 or lab[half] == 5:
    half += 1
  x1 = AO.planted_logits(rng, lab[:half], (T - forced) // 2, C)[0]
  x2 = AO.planted_logits(rng, lab[half:], T - forced - x1.shape[0], C)[0]
  mid = rng.standard_normal((forced, C)).astype(np.float32)
  mid[:, 5] += 8.0
  return np.concatenate([x1, mid, x2]), lab[:half] + [5] + lab[half:], half


def long_shape(rng, name, T, L, calls, forced=0):
  x, lab, forced_at = planted_text(rng, T, L, forced)
  d_x = torch.zeros((T, PITCH), dtype=torch.float32, device=DEV)
  d_x[:, :C] = to(x)
  stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
  keep, variants, out = [], {}, {}

  def variant(name, labels, wild, fit):
    n = len(labels)
    d_ids = to(np.array(labels + [0], dtype=np.int32))
    spans = torch.empty((n, 2), dtype=torch.int32, device=DEV)
    score = torch.empty(1, dtype=torch.float64, device=DEV)
    stat = torch.empty(1, dtype=torch.int32, device=DEV)
    fits = torch.empty(n, dtype=torch.float64, device=DEV)
    need = lib.st_ctc_align_long_ws(T, n)
    ws = torch.empty(need // 4 + 4, dtype=torch.int32, device=DEV)
    keep.append((d_ids, spans, score, stat, fits, ws))
    if wild:
      variants[name] = lambda: _lib.call('st_ctc_align_long_wild_f32', P(d_x), T, C, PITCH, P(d_ids), n, BIAS, P(spans), P(score), P(stat),
                                         P(fits) if fit else None, P(ws), need, stream)
    else:
      variants[name] = lambda: _lib.call('st_ctc_align_long_f32', P(d_x), T, C, PITCH, P(d_ids), n, P(spans), P(score), P(stat), P(ws), need,
                                         stream)
    out[name] = (spans, stat)

  variant('plain', lab, False, False)
  for vname, labels in (('no wildcard', lab), ('every 20th word', every_20th_word(lab)), ('ends only', ends_only(lab))):
    variant(vname, labels, True, False)
    variant(vname + ', fit', labels, True, True)
  times = alternating(variants, a.rounds, calls)
  assert all(int(s[1].cpu()[0]) == 0 for s in out.values())
  entry = dict(shape=name, output_frames=T, labels=len(lab), calls_per_round=calls, rounds=a.rounds, variants=summary(times),
               fit_stage={k: fit_stage(times, k) for k in ('no wildcard', 'every 20th word', 'ends only')})
  if forced:
    sp = out['no wildcard'][0].cpu().numpy()[forced_at]
    entry['forced_label_frames'] = int(sp[1] - sp[0])
  return entry


def existing_child():
  """One process: the existing paths of the tree this process imports (TREE), the smallest of 5 rounds each."""
  rng = np.random.default_rng(1)
  stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
  best = lambda fn, calls: min(alternating(dict(x=fn), 5, calls)['x'])
  res = {}
  # st_ctc_align_f32, 64 x 501
  B, T = 64, 501
  labs = [text_labels(rng, int(rng.integers(100, 151))) for _ in range(B)]
  lens = [len(l) for l in labs]
  offs = np.zeros(B + 1, dtype=np.int32)
  offs[1:] = np.cumsum(lens)
  x = torch.zeros((B, T, PITCH), dtype=torch.float32, device=DEV)
  x[:, :, :C] = to(np.stack([AO.random_logits(rng, T, C, 1.0) for _ in range(B)]))
  desc = Tensor3(x.data_ptr(), B, T, C, 0, T, PITCH)
  d_ids, d_offs, d_lens = to(np.array([i for l in labs for i in l] + [0], dtype=np.int32)), to(offs), to(np.full(B, T, dtype=np.int32))
  spans = torch.empty((int(offs[-1]), 2), dtype=torch.int32, device=DEV)
  score, stat = torch.empty(B, dtype=torch.float32, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
  need = lib.st_ctc_align_ws(B, T, max(lens))
  ws = torch.empty(need // 4 + 4, dtype=torch.int32, device=DEV)
  res['align_f32_us'] = best(lambda: _lib.call('st_ctc_align_f32', ctypes.byref(desc), P(d_ids), P(d_offs), P(d_lens), max(lens), P(spans), None,
                                               P(score), P(stat), P(ws), need, stream), 20)
  # st_ctc_align_ring_f32: 16 utterances of 300 rows kept in a ring (cap 310, first row 100), 30-45 labels
  J, R, cap, u0 = 16, 300, 310, 100
  labs = [text_labels(rng, int(rng.integers(30, 46))) for _ in range(J)]
  lens = [len(l) for l in labs]
  offs = np.zeros(J + 1, dtype=np.int32)
  offs[1:] = np.cumsum(lens)
  dense = torch.zeros((J, R, PITCH), dtype=torch.float32, device=DEV)
  dense[:, :, :C] = to(np.stack([AO.random_logits(rng, R, C, 1.0) for _ in range(J)]))
  ring = torch.zeros(J * cap * PITCH, dtype=torch.float32, device=DEV)
  table = to(np.array([(j, u0 + t) for j in range(J) for t in range(R)], dtype=np.int32))
  _lib.call('st_stream_keep_f32', P(dense), PITCH, C, P(table), J * R, J, P(ring), cap, None)
  d_jobs = to(np.array([(j, u0, R) for j in range(J)], dtype=np.int32))
  r_ids, r_offs = to(np.array([i for l in labs for i in l] + [0], dtype=np.int32)), to(offs)
  r_spans = torch.empty((int(offs[-1]), 2), dtype=torch.int32, device=DEV)
  r_score, r_stat = torch.empty(J, dtype=torch.float32, device=DEV), torch.empty(J, dtype=torch.int32, device=DEV)
  r_need = lib.st_ctc_align_ws(J, R, max(lens))
  r_ws = torch.empty(r_need // 4 + 4, dtype=torch.int32, device=DEV)
  res['align_ring_f32_us'] = best(lambda: _lib.call('st_ctc_align_ring_f32', P(ring), J, cap, C, P(d_jobs), J, R, P(r_ids), P(r_offs), max(lens),
                                                    P(r_spans), None, P(r_score), P(r_stat), P(r_ws), r_need, stream), 20)
  assert int(r_stat.abs().sum().cpu()) == 0 and int(stat.abs().sum().cpu()) == 0
  # st_ctc_align_long_f32, ten minutes
  xl, lab, _ = planted_text(rng, 41400, 9000)
  T, n = xl.shape[0], len(lab)
  d_x = torch.zeros((T, PITCH), dtype=torch.float32, device=DEV)
  d_x[:, :C] = to(xl)
  l_ids = to(np.array(lab + [0], dtype=np.int32))
  l_spans = torch.empty((n, 2), dtype=torch.int32, device=DEV)
  l_score, l_stat = torch.empty(1, dtype=torch.float64, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV)
  l_need = lib.st_ctc_align_long_ws(T, n)
  l_ws = torch.empty(l_need // 4 + 4, dtype=torch.int32, device=DEV)
  res['align_long_f32_us'] = best(lambda: _lib.call('st_ctc_align_long_f32', P(d_x), T, C, PITCH, P(l_ids), n, P(l_spans), P(l_score), P(l_stat),
                                                    P(l_ws), l_need, stream), 3)
  assert int(l_stat.cpu()[0]) == 0
  print('CHILD ' + json.dumps(res), flush=True)


def existing_paths(parent):
  """The existing paths of the parent's tree and of this one in fresh processes, alternating, the parent first in every pair."""
  runs = {'parent': [], 'this': []}
  for _ in range(a.repeats):
    for name, tree in (('parent', os.path.abspath(parent)), ('this', ROOT)):
      p = subprocess.run([sys.executable, os.path.abspath(__file__), '--existing-child', tree], capture_output=True, text=True, timeout=600)
      line = [l for l in p.stdout.splitlines() if l.startswith('CHILD ')]
      if p.returncode != 0 or not line:
        raise RuntimeError('existing-paths child of {} failed:\n{}'.format(tree, p.stdout[-2000:] + p.stderr[-2000:]))
      res = json.loads(line[0][6:])
      b = subprocess.run([sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5'], capture_output=True,
                         text=True, timeout=900, cwd=tree)
      if b.returncode != 0:
        raise RuntimeError('bench.py of {} failed:\n{}'.format(tree, b.stdout[-2000:] + b.stderr[-2000:]))
      res['bench_py_value'] = float(json.loads(b.stdout.strip().splitlines()[-1])['value'])
      runs[name].append(res)
      print(name, json.dumps(res), flush=True)
  med = lambda v: sorted(v)[len(v) // 2]
  paths = {}
  for k in runs['parent'][0]:
    pv, tv = [r[k] for r in runs['parent']], [r[k] for r in runs['this']]
    paths[k] = dict(parent=[round(v, 2) for v in pv], this=[round(v, 2) for v in tv], this_over_parent=round(med(tv) / med(pv), 4),
                    inside_parent_min_max=bool(min(pv) <= med(tv) <= max(pv)))
  return dict(repeats=a.repeats, order='the parent first in every pair',
              note='*_us: smallest of 5 rounds of a process, lower is better; bench_py_value: utterances/sec, higher is better', paths=paths)


if a.existing_child:
  existing_child()
  sys.exit(0)

rng = np.random.default_rng(0)
results = []
for entry in () if a.skip_new else (lambda: batch_shape(rng, 64, 501, 100, 150, 20), lambda: batch_shape(rng, 16, 1501, 300, 450, 20),
              lambda: long_shape(rng, 'ten minutes', 41400, 9000, 3),
              lambda: long_shape(rng, 'ten minutes, one label forced over 5 000 frames', 41400, 9000, 3, forced=5000)):
  results.append(entry())
  print(json.dumps(results[-1]), flush=True)
  torch.cuda.empty_cache()

out = dict(what='st_ctc_align_wild_f32 / st_ctc_align_long_wild_f32 (the plain lattice and back-trace kernels behind a softmax stage that '
                'also writes the wildcard\'s emission; with the fit, a row-maximum pass and one lane per label after the back-trace) beside '
                'st_ctc_align_f32 / st_ctc_align_long_f32 on the same logits; text-like labels, 29 classes, bias -1.0; random logits at '
                'the batch shapes, planted logits at the ten-minute shape',
           method='HIP events around back-to-back calls; every round times every variant once, in turn; us = median of the rounds, '
                  'over_plain = median (smallest, largest) of the rounds\' own ratios to the plain entry point on the unchanged labels; '
                  'fit_stage = fit on - fit off inside a round',
           device=torch.cuda.get_device_name(0), shapes=results)
if a.parent:
  out['existing_paths_vs_parent'] = existing_paths(a.parent)
os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
with open(a.output, 'w') as f:
  json.dump(out, f, indent=1)
  f.write('\n')
