#!/usr/bin/env python3
"""Scoring one generation of the LM weight search (`speecht-cli search`): the multi-candidate LM beam search against separate
single-candidate calls, the batched edit-distance kernel against the host scorer, and generations per second of the whole
scoring path (decode + statistics; the forward pass is not included).

Workload: B = 64 utterances of about 10 s (T' = 500 frames) of synthetic logits that spell words of the synthetic 200 k / 1 M /
1 M trigram of scripts/bench_lm_decode.py (its generator, imported), beam 100 on log10(softmax + 1e-8); the labels are the
spelled sentences themselves with every tenth word replaced (about 120 letters each).  Device times are HIP events around the
library calls.  Writes a JSON record (default profiles/lm_search.json)."""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from bench_lm_decode import LETTERS, synthetic_arpa, timed  # noqa: E402
from speecht_amd import _lib, vocabulary  # noqa: E402
from speecht_amd.candidate_scoring import score_candidates  # noqa: E402
from speecht_amd.engine import Wav2LetterEngine  # noqa: E402
from speecht_amd.language_model import LanguageModel  # noqa: E402
from speecht_amd.speech_input import SparseTensorValue  # noqa: E402


def spelled(seed, words, batch, frames):
  """[batch, frames, 29] logits spelling random frequent words, and the sentences they spell."""
  rng = np.random.default_rng(seed)
  out = rng.standard_normal((batch, frames, 29)).astype(np.float32)
  sentences = []
  for b in range(batch):
    t, text = 0, []
    while t + 4 * 3 < frames:
      w = words[min(int(rng.zipf(1.3)) - 1, len(words) - 1)]
      if t + 4 * (len(w) + 1) > frames:
        break
      for ch in w + ' ':
        out[b, t:t + 3, 27 if ch == ' ' else LETTERS.index(ch)] += 3.0
        out[b, t + 3:t + 4, 28] += 3.0
        t += 4
      text.append(w)
    sentences.append(text)
  return out, sentences


def sparse(rows):
  idx = [[b, p] for b, r in enumerate(rows) for p in range(len(r))]
  return SparseTensorValue(np.array(idx, dtype=np.int64).reshape(-1, 2), np.array([v for r in rows for v in r], dtype=np.int64),
                           np.array([len(rows), max([len(r) for r in rows] + [0])], dtype=np.int64))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=64)
  ap.add_argument('--frames', type=int, default=500)
  ap.add_argument('--beam', type=int, default=100)
  ap.add_argument('--candidates', type=str, default='1,4,16,64')
  ap.add_argument('--generation', type=int, default=16, help='candidates of the generation scored end to end')
  ap.add_argument('--samples', type=int, default=3)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lm_search.json'))
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  text, words = synthetic_arpa(1234, 200000, 1000000, 1000000)
  with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, 'synthetic.arpa')
    with open(path, 'w') as f:
      f.write(text)
    lm = LanguageModel(path)
  handle = lm.device_handle(dev)
  B, T, W = args.batch, args.frames, args.beam
  eng = Wav2LetterEngine([(1, 1, 16, 29, False)], device=dev)
  eng.load_batch(np.zeros((B, T, 16), dtype=np.float32), [T] * B)
  logits, sentences = spelled(77, words[:5000], B, T)
  eng.X[-1].interior().copy_(torch.as_tensor(logits))
  eng.ctc_lens = torch.full((B,), T, dtype=torch.int32, device=dev)
  rng = np.random.default_rng(5)
  labels = []
  for s in sentences:
    s = [words[int(rng.integers(0, 5000))] if i % 10 == 9 else w for i, w in enumerate(s)]
    labels.append(vocabulary.sentence_to_ids(' '.join(s)))
  label = sparse(labels)
  lib = _lib.load()
  eng._wait_uploads()
  w_rng = np.random.default_rng(9)

  def triples(P):
    return np.column_stack([1.0 + w_rng.normal(0, 0.5, P), w_rng.normal(0, 0.5, P), w_rng.normal(0, 0.5, P)]).astype(np.float32)

  # -- decode: one multi-candidate call against P single calls ---------------------------------------------------------------
  decode = {}
  for P in [int(p) for p in args.candidates.split(',')]:
    w = triples(P)
    chunk = P
    while chunk > 1 and lib.st_ctc_beam_lm_candidates_ws(B, T, W, chunk) > (1 << 30):
      chunk = (chunk + 1) // 2
    need = lib.st_ctc_beam_lm_candidates_ws(B, T, W, chunk)
    ws = eng._storage.view('beam_ws', need // 4 + 16, torch.int32)[0]
    ids = torch.empty(P * B * T, dtype=torch.int32, device=dev)
    lens = torch.empty(P * B, dtype=torch.int32, device=dev)
    lp = torch.empty(P * B, dtype=torch.float32, device=dev)

    def multi():
      for p0 in range(0, P, chunk):
        n = min(chunk, P - p0)
        wc = np.ascontiguousarray(w[p0:p0 + n])
        _lib.call('st_ctc_beam_search_decode_lm_candidates', eng.X[-1].ref, eng._ptr(eng.ctc_lens), W, 1, handle,
                  wc.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), n, ctypes.c_float(-1000.0),
                  ctypes.c_void_p(ids.data_ptr() + 4 * p0 * B * T), T, ctypes.c_void_p(lens.data_ptr() + 4 * p0 * B),
                  ctypes.c_void_p(lp.data_ptr() + 4 * p0 * B), eng._ptr(ws), ws.numel() * 4, eng.stream_ptr)

    def singles():
      for p in range(P):
        _lib.call('st_ctc_beam_search_decode_lm', eng.X[-1].ref, eng._ptr(eng.ctc_lens), W, 1, handle, ctypes.c_float(w[p, 0]),
                  ctypes.c_float(w[p, 1]), ctypes.c_float(w[p, 2]), ctypes.c_float(-1000.0), eng._ptr(eng.dec_ids), T,
                  eng._ptr(eng.dec_lens), eng._ptr(eng.dec_score), eng._ptr(ws), ws.numel() * 4, eng.stream_ptr)
    m, s = [], []
    for _ in range(args.samples):
      m.append(timed(multi, 1))
      s.append(timed(singles, 1))
    mm, sm = float(np.median(m)), float(np.median(s))
    decode[str(P)] = {'multi_ms': round(mm, 2), 'singles_ms': round(sm, 2), 'multi_per_candidate_ms': round(mm / P, 3),
                      'single_call_ms': round(sm / P, 3), 'per_candidate_over_single': round((mm / P) / (sm / P), 3),
                      'launches_of_64': -(-chunk // 64), 'python_chunks': -(-P // chunk)}
    print('P={}: {}'.format(P, decode[str(P)]), file=sys.stderr)

  # -- one generation: statistics on the device against the host scorer -----------------------------------------------------
  G = args.generation
  wg = triples(G)
  dec = eng.lm_beam_search_decode_candidates(lm, wg, W)
  torch.cuda.synchronize()
  n_pairs = G * B
  pairs = torch.as_tensor(np.array([(b, p * B + b) for p in range(G) for b in range(B)], dtype=np.int32)).to(dev)
  pitch = max(len(l) for l in labels)
  mat = np.zeros((B, pitch), dtype=np.int32)
  for b, l in enumerate(labels):
    mat[b, :len(l)] = l
  d_lab = torch.as_tensor(mat).to(dev)
  d_lab_lens = torch.as_tensor(np.array([len(l) for l in labels], dtype=np.int32)).to(dev)
  out = torch.empty(n_pairs * 2, dtype=torch.int32, device=dev)

  def edit():
    _lib.call('st_edit_distance_pairs', ctypes.c_void_p(d_lab.data_ptr()), B, pitch, ctypes.c_void_p(d_lab_lens.data_ptr()),
              ctypes.c_void_p(dec.ids.data_ptr()), G * B, T, ctypes.c_void_p(dec.lens.data_ptr()), ctypes.c_void_p(pairs.data_ptr()),
              n_pairs, ctypes.c_void_p(out.data_ptr()), eng.stream_ptr)
  edit_ms = float(np.median([timed(edit, 3) for _ in range(args.samples)]))
  t0 = time.perf_counter()
  host_stats = score_candidates(label, dec, pair_by_row=True, device=False)
  host_s = time.perf_counter() - t0
  t0 = time.perf_counter()
  dev_stats = score_candidates(label, dec, pair_by_row=True, device=True)
  dev_s = time.perf_counter() - t0
  same = all(a.__dict__ == b.__dict__ for a, b in zip(host_stats, dev_stats))

  # -- generations per second of the scoring path (decode + statistics) -------------------------------------------------------
  def generation():
    d = eng.lm_beam_search_decode_candidates(lm, triples(G), W)
    score_candidates(label, d, pair_by_row=True, device=True)
  generation()
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  reps = 3
  for _ in range(reps):
    generation()
  torch.cuda.synchronize()
  gen_s = (time.perf_counter() - t0) / reps
  rec = {'workload': 'B = {} utterances x T\' = {} frames (about 10 s), beam {}, log10(softmax + 1e-8) input'.format(B, T, W),
         'model': dict(lm.info, synthetic_seed=1234),
         'decode': decode,
         'generation': {'candidates': G, 'pairs': n_pairs, 'mean_label_letters': round(float(np.mean([len(l) for l in labels])), 1),
                        'edit_distance_kernel_ms': round(edit_ms, 3), 'host_scorer_s': round(host_s, 3),
                        'device_scorer_s': round(dev_s, 4), 'device_equals_host': same},
         'generations_per_s': round(1.0 / gen_s, 3), 'generation_s': round(gen_s, 3),
         'method': 'device times: median of {} samples between HIP events; host and end-to-end times: wall clock'.format(args.samples),
         'device': torch.cuda.get_device_name(0)}
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(rec, f, indent=1)
  print(json.dumps(rec))


if __name__ == '__main__':
  main()
