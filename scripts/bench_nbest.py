#!/usr/bin/env python3
"""N-best lists and sentence scores on the configs[4] shard (16 utterances of 30 s, T' = 1501), with HIP events around the
library calls on resident logits:

  - the top-path entry points (beam 16 LM-free, beam 100 with the synthetic trigram model of scripts/bench_lm_decode.py) of this
    build and, with ``--baseline-lib``, of another build of the library (the parent commit's), interleaved in one session: their
    kernels are meant to be the same code, so the two must agree within the spread of the baseline's own repeats;
  - the same shapes through the N-best entry points at n_best 1, 10 and 100 (capped at the beam), and the ratio to the top path;
  - st_lm_score_prefixes_f64 on 16 x 100 prefixes of 300-450 ids against its host form on one CPU thread.

Writes a JSON record (default profiles/nbest.json) that carries the digest of the sources it ran."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_lm_decode import LETTERS, spelled_logits, synthetic_arpa, timed  # noqa: E402
from speecht_amd import _lib  # noqa: E402
from speecht_amd.build import source_digest  # noqa: E402
from speecht_amd.engine import Wav2LetterEngine  # noqa: E402
from speecht_amd.language_model import LanguageModel  # noqa: E402

WEIGHTS = (0.8, 0.0, 2.3, -1000.0)


def baseline_library(path, arpa_bytes, stream_ptr):
  """Another build of the library and its own handle of the same model, uploaded to the same device."""
  lib = ctypes.CDLL(path)
  for name in ('st_ctc_beam_search_decode_ex', 'st_ctc_beam_search_decode_lm', 'st_lm_create_arpa', 'st_lm_upload'):
    res, args = _lib._SIGNATURES[name]
    getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
  handle = ctypes.c_void_p()
  err = ctypes.create_string_buffer(512)
  if lib.st_lm_create_arpa(arpa_bytes, len(arpa_bytes), ctypes.byref(handle), err, len(err)) != 0:
    raise RuntimeError(err.value.decode())
  if lib.st_lm_upload(handle, stream_ptr) != 0:
    raise RuntimeError('st_lm_upload failed in the baseline library')
  return lib, handle


def spread(samples):
  return dict(median=round(float(np.median(samples)), 4), min=round(float(min(samples)), 4), max=round(float(max(samples)), 4),
              all=[round(float(x), 4) for x in samples])


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=16)
  ap.add_argument('--frames', type=int, default=1501)
  ap.add_argument('--unigrams', type=int, default=200000)
  ap.add_argument('--bigrams', type=int, default=1000000)
  ap.add_argument('--trigrams', type=int, default=1000000)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--samples', type=int, default=7)
  ap.add_argument('--baseline-lib', default=None, help='libspeecht_hip.so of the build to compare the top-path entry points with')
  ap.add_argument('--baseline-name', default='parent commit')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nbest.json'))
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  text, words = synthetic_arpa(1234, args.unigrams, args.bigrams, args.trigrams)
  with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, 'synthetic.arpa')
    with open(path, 'w') as f:
      f.write(text)
    lm = LanguageModel(path)
  B, T = args.batch, args.frames
  eng = Wav2LetterEngine([(1, 1, 16, 29, False)], device=dev)
  eng.load_batch(np.zeros((B, T, 16), dtype=np.float32), [T] * B)
  eng.X[-1].interior().copy_(torch.as_tensor(spelled_logits(77, words[:5000], B, T)))
  eng.ctc_lens = torch.full((B,), T, dtype=torch.int32, device=dev)
  lib = _lib.load()
  ws = eng._storage.view('beam_ws', lib.st_ctc_beam_ws(B, eng.t_out, 128) // 4 + 16, torch.int32)[0]
  handle = lm.device_handle(dev)
  f32 = ctypes.c_float
  # outputs of the N-best calls: ids [B][100][T] | lens | log_prob | n_hyps
  nb_ids = torch.zeros(B * 100 * eng.t_out, dtype=torch.int32, device=dev)
  nb_lens = torch.zeros(B * 100, dtype=torch.int32, device=dev)
  nb_logp = torch.zeros(B * 100, dtype=torch.float32, device=dev)
  nb_count = torch.zeros(B, dtype=torch.int32, device=dev)
  eng._wait_uploads()
  torch.cuda.synchronize()
  top = (eng._ptr(eng.dec_ids), eng.t_out, eng._ptr(eng.dec_lens), eng._ptr(eng.dec_score), eng._ptr(ws), ws.numel() * 4, eng.stream_ptr)
  lists = (eng._ptr(nb_ids), eng.t_out, eng._ptr(nb_lens), eng._ptr(nb_logp), eng._ptr(nb_count), eng._ptr(ws), ws.numel() * 4,
           eng.stream_ptr)
  logits, lens = eng.X[-1].ref, eng._ptr(eng.ctc_lens)

  def checked(fn, *a):
    def run():
      if fn(*a) != 0:
        raise RuntimeError('a library call failed')
    return run

  runs = {'lm_free_beam16': checked(lib.st_ctc_beam_search_decode_ex, logits, lens, 16, 1, *top),
          'lm_beam100': checked(lib.st_ctc_beam_search_decode_lm, logits, lens, 100, 1, handle, *(f32(w) for w in WEIGHTS), *top)}
  if args.baseline_lib:
    base, base_handle = baseline_library(args.baseline_lib, text.encode(), eng.stream_ptr)
    runs['baseline_lm_free_beam16'] = checked(base.st_ctc_beam_search_decode_ex, logits, lens, 16, 1, *top)
    runs['baseline_lm_beam100'] = checked(base.st_ctc_beam_search_decode_lm, logits, lens, 100, 1, base_handle, *(f32(w) for w in WEIGHTS),
                                          *top)
  for n in (1, 10, 100):
    runs['lm_free_beam16_nbest{}'.format(min(n, 16))] = checked(lib.st_ctc_beam_search_decode_nbest, logits, lens, 16, 1, min(n, 16), *lists)
    runs['lm_beam100_nbest{}'.format(n)] = checked(lib.st_ctc_beam_search_decode_lm_nbest, logits, lens, 100, 1, handle,
                                                   *(f32(w) for w in WEIGHTS), n, *lists)
  ms = {k: [] for k in runs}
  with torch.cuda.stream(eng.stream):                 # (the events of `timed` go on the stream the calls run on)
    for _ in range(args.samples):                     # alternated, so that drift on a shared machine hits every variant alike
      for k, fn in runs.items():
        ms[k].append(timed(fn, args.reps))
  med = {k: float(np.median(v)) for k, v in ms.items()}

  # sentence scores: 16 x 100 prefixes of 300-450 ids spelling vocabulary words, device against host (one thread)
  rng = np.random.default_rng(5)
  prefixes = []
  for _ in range(16 * 100):
    want, ids = int(rng.integers(300, 451)), []
    while len(ids) < want:
      w = words[min(int(rng.zipf(1.3)) - 1, len(words) - 1)]
      ids += [LETTERS.index(ch) for ch in w] + [27]
    prefixes.append(ids[:want])
  n = len(prefixes)
  plens = np.array([len(p) for p in prefixes], dtype=np.int32)
  pitch = int(plens.max())
  pids = np.zeros((n, pitch), dtype=np.int32)
  for i, p in enumerate(prefixes):
    pids[i, :len(p)] = p
  d_ids, d_lens = torch.as_tensor(pids).to(dev), torch.as_tensor(plens).to(dev)
  d_g = torch.zeros(n, dtype=torch.float64, device=dev)
  d_w, d_v = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
  torch.cuda.synchronize()
  score_dev = checked(lib.st_lm_score_prefixes_f64, handle, eng._ptr(d_ids), pitch, eng._ptr(d_lens), n, eng._ptr(d_g), eng._ptr(d_w),
                      eng._ptr(d_v), eng.stream_ptr)
  with torch.cuda.stream(eng.stream):
    score_ms = [timed(score_dev, args.reps) for _ in range(args.samples)]
  h_g, h_w, h_v = np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32)
  ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
  host_ms = []
  for _ in range(args.samples):
    t0 = time.perf_counter()
    _lib.call('st_lm_score_prefixes_host', handle, ptr(pids), pitch, ptr(plens), n, ptr(h_g), ptr(h_w), ptr(h_v))
    host_ms.append((time.perf_counter() - t0) * 1e3)
  identical = bool(np.array_equal(d_g.cpu().numpy().view(np.int64), h_g.view(np.int64)) and np.array_equal(d_w.cpu().numpy(), h_w) and
                   np.array_equal(d_v.cpu().numpy(), h_v))

  rec = {'source_digest': source_digest(),
         'workload': 'configs[4] shard: batch {} x T\'={}, input log10(softmax + 1e-8)'.format(B, T),
         'model': dict(lm.info, synthetic_seed=1234),
         'ms_device': {k: spread(v) for k, v in ms.items()},
         'nbest_over_top_path': {k: round(med[k] / med[k.split('_nbest')[0]], 4) for k in med if '_nbest' in k},
         'sentence_scores': {'prefixes': n, 'ids_per_prefix': [int(plens.min()), int(plens.max())], 'device_ms': spread(score_ms),
                             'host_one_thread_ms': spread(host_ms), 'bit_identical': identical},
         'method': 'median (min, max) of {} samples, each the mean of {} back-to-back calls between HIP events (log-softmax rows + '
                   'search kernel), variants alternated'.format(args.samples, args.reps),
         'device': torch.cuda.get_device_name(0)}
  if args.baseline_lib:
    rec['baseline'] = args.baseline_name
    rec['top_path_over_baseline'] = {k: round(med[k] / med['baseline_' + k], 4) for k in ('lm_free_beam16', 'lm_beam100')}
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(rec, f, indent=1)
  print(json.dumps(rec))


if __name__ == '__main__':
  main()
