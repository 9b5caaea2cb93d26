#!/usr/bin/env python3
"""What SpecAugment on the device costs: `Wav2LetterEngine.load_batch` on a batch that already lives in HBM (what the input
pipeline hands the training step) at 32 x 1 001 x 80 and 64 x 1 654 x 128 with utterance lengths of 2 s up to the padded length,
  (a) plain (the strided copy into the padded input tensor),
  (b) with the identity policy (st_spec_augment_f32 moving the same bytes),
  (c) with the LD policy (time warp 80, 2 x 27 channels, 2 x 100 frames),
  (d) the whole fp32 training step (load_batch, forward, CTC, backward, update) without and with LD,
  (e) the device side alone: the bare strided copy against the bare st_spec_augment_f32 call, and the kernel's traced time,
and, as the yardstick for (a), the same plain load_batch of ANOTHER checkout -- the parent commit, built -- given with
--parent-root: it runs in child processes of this script before and after this tree's measurements, same shapes, same session.
HIP events around 20 back-to-back calls (5 steps for (d)), 7 rounds, the variants taking turns inside every round; each figure is
the median of the rounds, its spread (max - min) / median.  Writes profiles/spec_augment.json (--output)."""
import argparse, ctypes, json, os, subprocess, sys
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--output', default=None)
ap.add_argument('--parent-root', default=None, help='a built checkout of the parent commit: its plain load_batch is the yardstick')
ap.add_argument('--root', default=None, help='(child) the checkout to import speecht_amd from')
ap.add_argument('--plain-only', action='store_true', help='(child) time the plain load_batch alone and print one JSON line')
ap.add_argument('--rounds', type=int, default=7)
a = ap.parse_args()
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(a.root) if a.root else HERE
sys.path.insert(0, ROOT)
import torch
from speecht_amd import _lib
from speecht_amd.engine import Wav2LetterEngine
from tests import workloads as WL

DEV = 'cuda:0'
SHAPES = [(32, 1001, 80, 100.0), (64, 1654, 128, 1654 / 15.0)]          # batch, frames, channels, frames per second


class Staged:
  """A batch in device memory as the input pipeline hands it over (speech_input.StagedBatch)."""

  def __init__(self, tensor):
    self.tensor, self.event = tensor, torch.cuda.Event()
    self.event.record()


def lengths(B, T, fps, seed):
  lens = np.random.default_rng(seed).integers(int(2 * fps), T + 1, B)
  lens[0] = T
  return lens.astype(np.int64)


def timed(variants, rounds, calls):
  """variants: {name: fn}.  Every round times `calls` back-to-back calls of each variant in turn -> {name: [us per call]}."""
  for fn in variants.values():
    for _ in range(3):
      fn()
  torch.cuda.synchronize()
  out = {name: [] for name in variants}
  for _ in range(rounds):
    for name, fn in variants.items():
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(calls):
        fn()
      e1.record()
      torch.cuda.synchronize()
      out[name].append(e0.elapsed_time(e1) / calls * 1e3)
  return out


def summary(times):
  med = float(np.median(times))
  return dict(us=round(med, 2), spread=round((max(times) - min(times)) / med, 4), rounds_us=[round(t, 2) for t in times])


def plain_only():
  res = []
  for B, T, C, fps in SHAPES:
    eng = Wav2LetterEngine(WL.w2l_layers(C), device=DEV)
    x = Staged(torch.randn((B, T, C), device=DEV))
    lens = lengths(B, T, fps, 1)
    res.append(timed({'plain': lambda: eng.load_batch(x, lens)}, a.rounds, 20)['plain'])
  print('PLAIN ' + json.dumps(res), flush=True)


def parent_plain():
  cmd = [sys.executable, os.path.abspath(__file__), '--plain-only', '--root', a.parent_root, '--rounds', str(a.rounds)]
  r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
  lines = [l for l in r.stdout.splitlines() if l.startswith('PLAIN ')]
  if r.returncode != 0 or not lines:
    raise RuntimeError('the parent checkout\'s run failed:\n' + r.stdout + r.stderr)
  return json.loads(lines[-1][6:])


def main():
  from speecht_amd import augmentation as A
  from speecht_amd.build import source_digest
  parent = [parent_plain()] if a.parent_root else []
  shapes = []
  for si, (B, T, C, fps) in enumerate(SHAPES):
    eng = Wav2LetterEngine(WL.w2l_layers(C), device=DEV)
    eng.init_xavier(3)
    x = Staged(torch.randn((B, T, C), device=DEV))
    lens = lengths(B, T, fps, 1)
    ids = A.draw_ids(0, B)
    identity, ld = A.SpecAugment(A.IDENTITY, 1, ids), A.SpecAugment('LD', 1, ids)
    load = timed({'plain': lambda: eng.load_batch(x, lens), 'identity': lambda: eng.load_batch(x, lens, augment=identity),
                  'LD': lambda: eng.load_batch(x, lens, augment=ld)}, a.rounds, 20)
    eng.load_batch(x, lens, augment=ld)
    plan = eng.augment_plan.cpu().numpy()
    # (e) the device side alone: the bare strided copy and the bare library call, 50 back to back, and the kernel's own time from the
    # library's timed launch trace (the dispatch's begin and end time stamps)
    X0, interior = eng.shape.X[0], eng.shape.X[0].interior()
    d_ids, d_lens = torch.as_tensor(ids).to(DEV), torch.as_tensor(lens.astype(np.int32)).to(DEV)
    d_plan = torch.empty((B, 10), dtype=torch.int32, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def kernel(policy, plan_out=None):
      _lib.call('st_spec_augment_f32', P(x.tensor), B, T, C, P(d_lens), P(d_ids), 1, *policy.c_args(), X0.ref,
                P(plan_out) if plan_out is not None else None, eng.stream_ptr)
    bare = timed({'copy': lambda: interior.copy_(x.tensor, non_blocking=True), 'identity': lambda: kernel(A.IDENTITY),
                  'LD': lambda: kernel(A.POLICIES['LD'], d_plan)}, a.rounds, 50)
    traced = {}
    warp_only, masks_only = A.SpecAugmentPolicy(80, 0, 0, 0, 0, 1.0), A.SpecAugmentPolicy(0, 27, 2, 100, 2, 1.0)
    for name, policy in (('identity', A.IDENTITY), ('LD', A.POLICIES['LD']), ('warp_only', warp_only), ('masks_only', masks_only)):
      with _lib.launch_trace(timed=True, only='spec_augment') as tr:
        for _ in range(10):
          kernel(policy, d_plan if name == 'LD' else None)
      traced[name] = sorted(float(l.split(' ms=')[1]) * 1e3 for l in tr.lines if ' ms=' in l)
    labels = [WL.make_labels(b, int(0.1 * l), int(l) // 2) for b, l in enumerate(lens)]

    def step(augment):
      eng.load_batch(x, lens, augment=augment) if augment is not None else eng.load_batch(x, lens)
      eng.set_labels(labels)
      eng.forward()
      eng.ctc_loss_grad(1.0 / B)
      eng.backward()
      eng.apply_update(lr=1e-5)
    steps = timed({'plain': lambda: step(None), 'LD': lambda: step(ld)}, a.rounds, 5)
    shapes.append(dict(batch=B, frames=T, channels=C, lengths_frames=[int(lens.min()), int(lens.max())], mean_length=float(lens.mean()),
                       bytes_read=B * T * C * 4, bytes_written=B * T * C * 4,
                       warped_utterances=int((plan[:, 0] > 0).sum()), masked_frames_mean=float(plan[:, 7::2].sum(1).mean()),
                       load_batch_plain=summary(load['plain']), load_batch_identity=summary(load['identity']),
                       load_batch_LD=summary(load['LD']),
                       device_only=dict(torch_copy=summary(bare['copy']), kernel_identity=summary(bare['identity']), kernel_LD=summary(bare['LD']),
                                        kernel_identity_traced_us=[round(t, 2) for t in traced['identity']],
                                        kernel_LD_traced_us=[round(t, 2) for t in traced['LD']],
                                        kernel_LD_warp_only_traced_us=[round(t, 2) for t in traced['warp_only']],
                                        kernel_LD_masks_only_traced_us=[round(t, 2) for t in traced['masks_only']]),
                       step_plain=summary(steps['plain']), step_LD=summary(steps['LD']), _load=load, _si=si))
  if a.parent_root:
    parent.append(parent_plain())
  for sh in shapes:
    load, si = sh.pop('_load'), sh.pop('_si')
    med = lambda v: float(np.median(v))
    if parent:
      runs = [p[si] for p in parent]
      every = [t for r in runs for t in r]
      sh['parent_load_batch_plain'] = dict(summary(every), process_medians_us=[round(med(r), 2) for r in runs])
      base = med(every)
      sh['ratios_to_parent_plain'] = {k: round(med(load[k]) / base, 4) for k in ('plain', 'identity', 'LD')}
    else:
      sh['parent_load_batch_plain'] = 'not measured (no --parent-root)'
    sh['ratios_to_plain'] = {k: round(med(load[k]) / med(load['plain']), 4) for k in ('identity', 'LD')}
    sh['step_LD_over_plain'] = round(sh['step_LD']['us'] / sh['step_plain']['us'], 4)
    print(json.dumps(sh), flush=True)
  out = dict(what='load_batch on a device-resident fp32 batch: plain (torch strided copy), identity policy and LD through '
                  'st_spec_augment_f32 (one launch + one pinned upload of lengths and draw ids, which the compute stream waits for), and '
                  'the fp32 training step without and with LD; device_only: 50 back-to-back bare copies / bare library calls (no uploads, no '
                  'Python around them) and the time of the kernel from the timed launch trace; parent_load_batch_plain is the plain load_batch of the parent commit, '
                  'run in two child processes before and after, same shapes and lengths',
             method='HIP events on the compute stream around 20 back-to-back load_batch calls (5 steps), {} rounds with the variants '
                    'taking turns; us = median of the rounds, spread = (max - min) / median'.format(a.rounds),
             device=torch.cuda.get_device_name(0), source_digest=source_digest(), shapes=shapes)
  path = a.output or os.path.join(HERE, 'profiles', 'spec_augment.json')
  os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
  with open(path, 'w') as f:
    json.dump(out, f, indent=1)
    f.write('\n')


if __name__ == '__main__':
  plain_only() if a.plain_only else main()
