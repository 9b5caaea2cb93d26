#!/usr/bin/env python3
"""Hotword biasing on the configs[4] shard (16 utterances of 30 s, T' = 1501), with HIP events around the library calls on resident
logits (the method of scripts/bench_nbest.py):

  - the biased searches (beam 16 LM-free; beam 100 with the synthetic trigram model of scripts/bench_lm_decode.py) at n_best = 1 with
    100 and 1 000 phrases of 5-15 ids, against the same search's n_best = 1 without hotwords, interleaved in one session;
  - the four existing beam entry points (top path and N-best, LM-free and LM) of this build and, with ``--baseline-lib``, of another
    build of the library (the parent commit's), interleaved: they compile from unchanged instantiations, so the two must agree
    within the spread of the baseline's own repeats;
  - the host's table build and upload for 1 000 phrases.

Writes a JSON record (default profiles/hotwords.json) that carries the digest of the sources it ran."""
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
from bench_lm_decode import spelled_logits, synthetic_arpa, timed  # noqa: E402
from bench_nbest import WEIGHTS, spread  # noqa: E402
from speecht_amd import _lib  # noqa: E402
from speecht_amd.build import source_digest  # noqa: E402
from speecht_amd.engine import Wav2LetterEngine  # noqa: E402
from speecht_amd.hotwords import Hotwords  # noqa: E402
from speecht_amd.language_model import LanguageModel  # noqa: E402

EXISTING = ('st_ctc_beam_search_decode_ex', 'st_ctc_beam_search_decode_lm', 'st_ctc_beam_search_decode_nbest',
            'st_ctc_beam_search_decode_lm_nbest')


def baseline_library(path, arpa_bytes, stream_ptr):
  """Another build of the library and its own handle of the same model, uploaded to the same device."""
  lib = ctypes.CDLL(path)
  for name in EXISTING + ('st_lm_create_arpa', 'st_lm_upload'):
    res, args = _lib._SIGNATURES[name]
    getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
  handle = ctypes.c_void_p()
  err = ctypes.create_string_buffer(512)
  if lib.st_lm_create_arpa(arpa_bytes, len(arpa_bytes), ctypes.byref(handle), err, len(err)) != 0:
    raise RuntimeError(err.value.decode())
  if lib.st_lm_upload(handle, stream_ptr) != 0:
    raise RuntimeError('st_lm_upload failed in the baseline library')
  return lib, handle


def phrases_from(words, count, seed):
  """`count` distinct phrases of 5-15 characters: one or two vocabulary words (the text the logits spell is drawn from the same
  words, so the phrases do match in places), cut to length."""
  rng = np.random.default_rng(seed)
  out = set()
  while len(out) < count:
    text = ' '.join(words[int(rng.integers(0, 5000))] for _ in range(2))
    text = text[:int(rng.integers(5, 16))].strip()
    if len(text) >= 5:
      out.add(text)
  return sorted(out)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=16)
  ap.add_argument('--frames', type=int, default=1501)
  ap.add_argument('--unigrams', type=int, default=200000)
  ap.add_argument('--bigrams', type=int, default=1000000)
  ap.add_argument('--trigrams', type=int, default=1000000)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--samples', type=int, default=7)
  ap.add_argument('--weight', type=float, default=1.0)
  ap.add_argument('--baseline-lib', default=None, help='libspeecht_hip.so of the build to compare the existing entry points with')
  ap.add_argument('--baseline-name', default='parent commit')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hotwords.json'))
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
  nb_ids = torch.zeros(B * eng.t_out, dtype=torch.int32, device=dev)
  nb_lens = torch.zeros(B, dtype=torch.int32, device=dev)
  nb_logp = torch.zeros(B, dtype=torch.float32, device=dev)
  nb_count = torch.zeros(B, dtype=torch.int32, device=dev)
  eng._wait_uploads()
  torch.cuda.synchronize()
  top = (eng._ptr(eng.dec_ids), eng.t_out, eng._ptr(eng.dec_lens), eng._ptr(eng.dec_score), eng._ptr(ws), ws.numel() * 4, eng.stream_ptr)
  lists = (eng._ptr(nb_ids), eng.t_out, eng._ptr(nb_lens), eng._ptr(nb_logp), eng._ptr(nb_count), eng._ptr(ws), ws.numel() * 4,
           eng.stream_ptr)
  logits, lens = eng.X[-1].ref, eng._ptr(eng.ctc_lens)
  lmw = tuple(f32(w) for w in WEIGHTS)

  def checked(fn, *a):
    def run():
      if fn(*a) != 0:
        raise RuntimeError('a library call failed')
    return run

  def existing(l, h, prefix=''):
    return {prefix + 'lm_free_beam16': checked(l.st_ctc_beam_search_decode_ex, logits, lens, 16, 1, *top),
            prefix + 'lm_beam100': checked(l.st_ctc_beam_search_decode_lm, logits, lens, 100, 1, h, *lmw, *top),
            prefix + 'lm_free_beam16_nbest1': checked(l.st_ctc_beam_search_decode_nbest, logits, lens, 16, 1, 1, *lists),
            prefix + 'lm_beam100_nbest1': checked(l.st_ctc_beam_search_decode_lm_nbest, logits, lens, 100, 1, h, *lmw, 1, *lists)}

  runs = existing(lib, handle)
  if args.baseline_lib:
    base, base_handle = baseline_library(args.baseline_lib, text.encode(), eng.stream_ptr)
    runs.update(existing(base, base_handle, 'baseline_'))
  # the host side: table build and upload for the phrase lists
  builder, keep, texts = {}, [], {}
  for count in (100, 1000):
    phrases = phrases_from(words, count, count)
    build_ms, upload_ms = [], []
    for _ in range(args.samples):
      t0 = time.perf_counter()
      hw = Hotwords(phrases, args.weight)
      t1 = time.perf_counter()
      tabs = hw.device_tables(dev)
      torch.cuda.synchronize()
      build_ms.append((t1 - t0) * 1e3)
      upload_ms.append((time.perf_counter() - t1) * 1e3)
    builder[str(count)] = dict(states=hw.n_states, table_bytes=int(hw.next.nbytes + hw.gain.nbytes + hw.fin.nbytes),
                               build_ms=spread(build_ms), upload_ms=spread(upload_ms))
    struct = _lib.BiasTables(tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), hw.n_states)
    keep.append((hw, tabs, struct))
    bias = ctypes.byref(struct)
    runs['lm_free_beam16_hot{}'.format(count)] = checked(lib.st_ctc_beam_search_decode_bias_nbest, logits, lens, 16, 1, bias, 1, *lists)
    runs['lm_beam100_hot{}'.format(count)] = checked(lib.st_ctc_beam_search_decode_lm_bias_nbest, logits, lens, 100, 1, handle, *lmw,
                                                     bias, 1, *lists)
    texts[count] = hw
  ms = {k: [] for k in runs}
  with torch.cuda.stream(eng.stream):                 # (the events of `timed` go on the stream the calls run on)
    for _ in range(args.samples):                     # alternated, so that drift on a shared machine hits every variant alike
      for k, fn in runs.items():
        ms[k].append(timed(fn, args.reps))
  med = {k: float(np.median(v)) for k, v in ms.items()}
  # what the bias did to the transcripts: characters credited in the winners, with and without
  credit = {}
  for count, hw in texts.items():
    for kind, beam, call in (('lm_free_beam16', 16, lambda **kw: eng.beam_search_decode_nbest(1, 16, 'log10_softmax', **kw)),
                             ('lm_beam100', 100, lambda **kw: eng.lm_beam_search_decode_nbest(lm, 1, 100, **kw))):
      plain, hot = call(), call(hotwords=hw)
      credit['{}_hot{}'.format(kind, count)] = dict(
          biased=round(sum(hw.score(l[0][0])[1] for l in hot), 1), unbiased=round(sum(hw.score(l[0][0])[1] for l in plain), 1),
          transcripts_changed=sum(a[0][0] != b[0][0] for a, b in zip(plain, hot)))

  rec = {'source_digest': source_digest(),
         'workload': 'configs[4] shard: batch {} x T\'={}, input log10(softmax + 1e-8); phrases of 5-15 characters drawn from the '
                     'vocabulary the logits spell, weight {}'.format(B, T, args.weight),
         'model': dict(lm.info, synthetic_seed=1234),
         'ms_device': {k: spread(v) for k, v in ms.items()},
         'biased_over_unbiased_nbest1': {k: round(med[k] / med[k.split('_hot')[0] + '_nbest1'], 4) for k in med if '_hot' in k},
         'final_credit_of_the_winners': credit,
         'tables': builder,
         'method': 'median (min, max) of {} samples, each the mean of {} back-to-back calls between HIP events (log-softmax rows + '
                   'search kernel), variants alternated; host times: time.perf_counter around Hotwords(...) and the first '
                   'device_tables'.format(args.samples, args.reps),
         'device': torch.cuda.get_device_name(0)}
  if args.baseline_lib:
    rec['baseline'] = args.baseline_name
    names = ('lm_free_beam16', 'lm_beam100', 'lm_free_beam16_nbest1', 'lm_beam100_nbest1')
    rec['existing_over_baseline'] = {k: round(med[k] / med['baseline_' + k], 4) for k in names}
    rec['spread_max_over_min'] = {k: round(max(ms[k]) / min(ms[k]), 4) for k in names + tuple('baseline_' + n for n in names)}
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(rec, f, indent=1)
  print(json.dumps(rec))


if __name__ == '__main__':
  main()
