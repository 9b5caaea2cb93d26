#!/usr/bin/env python3
"""st_ctc_loss_grad_wild_f32 beside st_ctc_loss_grad_hilo_f32, in one session, alternating round by round on the same logits:
  32 x 501 output frames with 100-150 labels, 16 x 1 501 output frames with 300-450 labels (random logits), 29 classes.
Labels are text-like: words of 2-9 letters with the space id between them.  Each shape runs the plain entry point on the labels
as they are, and the wildcard entry point on the same labels (no wildcard in any label: the same lattice and the same bits), with
a wildcard and a space added at both ends, and with every 20th word replaced by one wildcard.  HIP events around back-to-back
calls; a round times every variant once, so a ratio is taken inside a round; reported: the median of the rounds' ratios with
their smallest and largest.  Writes profiles/ctc_wild.json (--output).

--parent TREE (a built tree of the parent commit): also st_ctc_loss_grad_hilo_f32 and bench.py of both trees, in fresh processes
that alternate, the parent first in every pair (--this-first: the other way round)."""
import argparse, ctypes, json, os, subprocess, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'ctc_wild.json'))
ap.add_argument('--rounds', type=int, default=9)
ap.add_argument('--parent', default=None, help='a built tree of the parent commit: also the existing paths of both trees, processes alternating')
ap.add_argument('--repeats', type=int, default=3, help='--parent: processes per tree')
ap.add_argument('--this-first', action='store_true', help='--parent: this tree first in every pair (default: the parent first)')
ap.add_argument('--existing-child', default=None, metavar='TREE', help='(internal) measure the existing path of TREE, print one JSON line')
a = ap.parse_args()
TREE = os.path.abspath(a.existing_child) if a.existing_child else ROOT
sys.path.insert(0, TREE)
from speecht_amd import _lib
from speecht_amd._lib import Tensor3

C, PITCH, SPACE, W = 29, 32, 27, 29
BIAS = -1.0
DEV = 'cuda:0'
lib = _lib.load()
P = lambda t: ctypes.c_void_p(t.data_ptr())
to = lambda x: torch.as_tensor(np.ascontiguousarray(x)).to(DEV)
SHAPES = ((32, 501, 100, 150), (16, 1501, 300, 450))


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


def make_shape(rng, B, T, lo, hi):
  labs = [text_labels(rng, int(rng.integers(lo, hi + 1))) for _ in range(B)]
  x = torch.zeros((B, T, PITCH), dtype=torch.float32, device=DEV)
  x[:, :, :C] = to((rng.standard_normal((B, T, C))).astype(np.float32))
  grad = torch.empty((B, T, PITCH), dtype=torch.float32, device=DEV)
  return labs, x, grad


def variant(keep, x, grad, labels, wild):
  B, T = x.shape[0], x.shape[1]
  lens = [len(l) for l in labels]
  offs = np.zeros(B + 1, dtype=np.int32)
  offs[1:] = np.cumsum(lens)
  max_len = max(lens)
  d_ids, d_offs, d_lens = to(np.array([i for l in labels for i in l] + [0], dtype=np.int32)), to(offs), to(np.full(B, T, dtype=np.int32))
  loss, lo_ = torch.empty(B, dtype=torch.float32, device=DEV), torch.empty(B, dtype=torch.float32, device=DEV)
  stat = torch.empty(B, dtype=torch.int32, device=DEV)
  need = lib.st_ctc_ws(B, T, max_len)
  ws = torch.empty(need // 4 + 4, dtype=torch.float32, device=DEV)
  xd, gd = Tensor3(x.data_ptr(), B, T, C, 0, T, PITCH), Tensor3(grad.data_ptr(), B, T, C, 0, T, PITCH)
  stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
  keep.append((d_ids, d_offs, d_lens, loss, lo_, stat, ws, xd, gd))
  head = (ctypes.byref(xd), P(d_ids), P(d_offs), P(d_lens), max_len, 1.0 / B)
  rest = (P(loss), P(lo_), ctypes.byref(gd), P(stat), P(ws), need, stream)
  if wild:
    return (lambda: _lib.call('st_ctc_loss_grad_wild_f32', *head, BIAS, *rest)), stat
  return (lambda: _lib.call('st_ctc_loss_grad_hilo_f32', *head, *rest)), stat


def batch_shape(rng, B, T, lo, hi, calls):
  labs, x, grad = make_shape(rng, B, T, lo, hi)
  keep, variants, status = [], {}, {}
  for name, labels, wild in (('plain', labs, False), ('no wildcard', labs, True), ('ends only', [ends_only(l) for l in labs], True),
                             ('every 20th word', [every_20th_word(l) for l in labs], True)):
    variants[name], status[name] = variant(keep, x, grad, labels, wild)
  times = alternating(variants, a.rounds, calls)
  assert all(int(s.abs().sum().cpu()) == 0 for s in status.values())
  return dict(batch=B, output_frames=T, label_lengths=[lo, hi], calls_per_round=calls, rounds=a.rounds, variants=summary(times))


def existing_child():
  """One process: st_ctc_loss_grad_hilo_f32 of the tree this process imports (TREE) at both shapes, the smallest of 5 rounds."""
  rng = np.random.default_rng(1)
  res = {}
  for B, T, lo, hi in SHAPES:
    labs, x, grad = make_shape(rng, B, T, lo, hi)
    keep = []
    fn, stat = variant(keep, x, grad, labs, False)
    res['hilo_{}x{}_us'.format(B, T)] = min(alternating(dict(x=fn), 5, 20)['x'])
    assert int(stat.abs().sum().cpu()) == 0
  print('CHILD ' + json.dumps(res), flush=True)


def existing_paths(parent):
  runs = {'parent': [], 'this': []}
  for _ in range(a.repeats):
    for name, tree in (('parent', os.path.abspath(parent)), ('this', ROOT))[::-1 if a.this_first else 1]:
      p = subprocess.run([sys.executable, os.path.abspath(__file__), '--existing-child', tree], capture_output=True, text=True, timeout=300)
      line = [l for l in p.stdout.splitlines() if l.startswith('CHILD ')]
      if p.returncode != 0 or not line:
        raise RuntimeError('existing-path child of {} failed:\n{}'.format(tree, p.stdout[-2000:] + p.stderr[-2000:]))
      res = json.loads(line[0][6:])
      b = subprocess.run([sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5'], capture_output=True,
                         text=True, timeout=600, cwd=tree)
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
  return dict(repeats=a.repeats, order='this tree first in every pair' if a.this_first else 'the parent first in every pair',
              note='*_us: smallest of 5 rounds of a process, lower is better; bench_py_value: higher is better', paths=paths)


if a.existing_child:
  existing_child()
  sys.exit(0)

rng = np.random.default_rng(0)
results = []
for B, T, lo, hi in SHAPES:
  results.append(batch_shape(rng, B, T, lo, hi, 20))
  print(json.dumps(results[-1]), flush=True)
  torch.cuda.empty_cache()

out = dict(what='st_ctc_loss_grad_wild_f32 (the plain recursion kernel behind a softmax stage that also writes the wildcard\'s emission, '
                'and a gradient kernel that also sums the wildcard states\' occupancy and hands it to the label classes) beside '
                'st_ctc_loss_grad_hilo_f32 on the same logits; text-like labels, 29 classes, bias -1.0, random logits',
           method='HIP events around back-to-back calls; every round times every variant once, in turn; us = median of the rounds, '
                  'over_plain = median (smallest, largest) of the rounds\' own ratios to the plain entry point on the unchanged labels',
           device=torch.cuda.get_device_name(0), shapes=results)
if a.parent:
  out['existing_paths_vs_parent'] = existing_paths(a.parent)
os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
with open(a.output, 'w') as f:
  json.dump(out, f, indent=1)
  f.write('\n')
