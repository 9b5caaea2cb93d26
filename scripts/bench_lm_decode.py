#!/usr/bin/env python3
"""The LM-scored prefix beam search on the configs[4] shard (16 utterances of 30 s, T' = 1501) against the LM-free search, with
HIP events around the library calls on resident logits; plus the cost of loading a language model (parse + tables + upload).

The model is a synthetic ARPA trigram of a realistic size generated from a fixed seed (200 k unigrams, 1 M bigrams, 1 M
trigrams, backoffs on most of the lower orders); the logits spell random vocabulary words (a peak of N(0, 1) noise + 3 per
character, 3 frames each, a blank frame between characters), so the search walks the trie and queries the n-grams the way it
does on speech.  Writes a JSON record (default profiles/lm_decode_config5.json)."""
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
from speecht_amd import _lib  # noqa: E402
from speecht_amd.engine import Wav2LetterEngine  # noqa: E402
from speecht_amd.language_model import LanguageModel  # noqa: E402

LETTERS = "abcdefghijklmnopqrstuvwxyz'"


def synthetic_arpa(seed, unigrams, bigrams, trigrams):
  rng = np.random.default_rng(seed)
  lens = rng.integers(2, 10, unigrams * 2)
  chars = rng.integers(0, 26, int(lens.sum()))
  words, pos = [], 0
  seen = set()
  for n in lens:
    w = ''.join(LETTERS[c] for c in chars[pos:pos + n])
    pos += n
    if w not in seen:
      seen.add(w)
      words.append(w)
      if len(words) == unigrams:
        break
  V = len(words)
  # Zipf-like unigram log10 probabilities: frequent words are short-listed first
  uni = -np.log10(np.arange(1, V + 1) * 1.0) - 1.0 + rng.uniform(-0.3, 0.3, V)

  def grams(count, base, width):
    # `count` distinct tuples extending `base` rows by a word drawn from the frequent end of the vocabulary
    keys = np.zeros(0, dtype=np.int64)                  # a tuple as one integer (V^3 < 2^63)
    while len(keys) < count:
      need = int((count - len(keys)) * 1.2) + 16
      rows = base[rng.integers(0, len(base), need)]
      nxt = np.minimum(rng.zipf(1.3, need) - 1, V - 1)
      k = nxt.astype(np.int64)
      for j in range(width - 1):
        k = k + rows[:, width - 2 - j].astype(np.int64) * V ** (j + 1)
      keys = np.unique(np.concatenate([keys, k]))
    keys = keys[rng.permutation(len(keys))[:count]]
    return np.stack([(keys // V ** (width - 1 - j)) % V for j in range(width)], axis=1)
  heads = np.minimum(rng.zipf(1.2, bigrams) - 1, V - 1)[:, None]
  big = grams(bigrams, heads, 2)
  tri = grams(trigrams, big, 3)
  fmt = lambda a: np.char.mod('%.4f', a)
  w = np.array(words)
  lines = ['\\data\\', 'ngram 1={}'.format(V + 3), 'ngram 2={}'.format(len(big)), 'ngram 3={}'.format(len(tri)), '', '\\1-grams:',
           '-1.5000\t</s>', '-99\t<s>\t-0.5000', '-5.0000\t<unk>']
  ubo = fmt(-rng.uniform(0.05, 1.0, V))
  lines += list(np.char.add(np.char.add(np.char.add(fmt(uni), '\t'), w), np.char.add('\t', ubo)))
  lines += ['', '\\2-grams:']
  bp, bbo = fmt(-rng.uniform(0.1, 2.5, len(big))), fmt(-rng.uniform(0.05, 1.0, len(big)))
  lines += list(np.char.add(np.char.add(np.char.add(np.char.add(np.char.add(bp, '\t'), w[big[:, 0]]), ' '), w[big[:, 1]]),
                            np.char.add('\t', bbo)))
  lines += ['', '\\3-grams:']
  tp = fmt(-rng.uniform(0.05, 2.0, len(tri)))
  lines += list(np.char.add(np.char.add(np.char.add(np.char.add(np.char.add(tp, '\t'), w[tri[:, 0]]), ' '),
                                        np.char.add(np.char.add(w[tri[:, 1]], ' '), w[tri[:, 2]])), ''))
  lines += ['', '\\end\\', '']
  return '\n'.join(lines), words


def spelled_logits(seed, words, batch, frames):
  """[batch, frames, 29] logits spelling random frequent words separated by spaces."""
  rng = np.random.default_rng(seed)
  out = rng.standard_normal((batch, frames, 29)).astype(np.float32)
  for b in range(batch):
    t = 0
    while t < frames:
      w = words[min(int(rng.zipf(1.3)) - 1, len(words) - 1)] + ' '
      for ch in w:
        c = 27 if ch == ' ' else LETTERS.index(ch)
        out[b, t:t + 3, c] += 3.0
        out[b, t + 3:t + 4, 28] += 3.0
        t += 4
        if t >= frames:
          break
  return out


def timed(fn, reps):
  fn()
  torch.cuda.synchronize()
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(reps):
    fn()
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b) / reps


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=16)
  ap.add_argument('--frames', type=int, default=1501)
  ap.add_argument('--unigrams', type=int, default=200000)
  ap.add_argument('--bigrams', type=int, default=1000000)
  ap.add_argument('--trigrams', type=int, default=1000000)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--samples', type=int, default=5)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lm_decode_config5.json'))
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  t0 = time.perf_counter()
  text, words = synthetic_arpa(1234, args.unigrams, args.bigrams, args.trigrams)
  t_gen = time.perf_counter() - t0
  with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, 'synthetic.arpa')
    with open(path, 'w') as f:
      f.write(text)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lm = LanguageModel(path)
    t_parse = time.perf_counter() - t0
    t0 = time.perf_counter()
    lm.device_handle(dev)
    torch.cuda.synchronize()
    t_upload = time.perf_counter() - t0
  B, T = args.batch, args.frames
  eng = Wav2LetterEngine([(1, 1, 16, 29, False)], device=dev)
  eng.load_batch(np.zeros((B, T, 16), dtype=np.float32), [T] * B)
  eng.X[-1].interior().copy_(torch.as_tensor(spelled_logits(77, words[:5000], B, T)))
  eng.ctc_lens = torch.full((B,), T, dtype=torch.int32, device=dev)
  lib = _lib.load()
  ws = eng._storage.view('beam_ws', lib.st_ctc_beam_ws(B, eng.t_out, 128) // 4 + 16, torch.int32)[0]
  handle = lm.device_handle(dev)
  eng._wait_uploads()

  def free(beam):
    return lambda: _lib.call('st_ctc_beam_search_decode_ex', eng.X[-1].ref, eng._ptr(eng.ctc_lens), beam, 1, eng._ptr(eng.dec_ids),
                             eng.t_out, eng._ptr(eng.dec_lens), eng._ptr(eng.dec_score), eng._ptr(ws), ws.numel() * 4, eng.stream_ptr)

  def with_lm(beam):
    return lambda: _lib.call('st_ctc_beam_search_decode_lm', eng.X[-1].ref, eng._ptr(eng.ctc_lens), beam, 1, handle,
                             ctypes.c_float(0.8), ctypes.c_float(0.0), ctypes.c_float(2.3), ctypes.c_float(-1000.0),
                             eng._ptr(eng.dec_ids), eng.t_out, eng._ptr(eng.dec_lens), eng._ptr(eng.dec_score), eng._ptr(ws),
                             ws.numel() * 4, eng.stream_ptr)
  runs = {'lm_free_beam16': free(16), 'lm_free_beam100': free(100), 'lm_beam100': with_lm(100)}
  ms = {k: [] for k in runs}
  for _ in range(args.samples):                       # alternated, so that drift on a shared machine hits every variant alike
    for k, fn in runs.items():
      ms[k].append(timed(fn, args.reps))
  med = {k: float(np.median(v)) for k, v in ms.items()}
  ids, _ = eng.lm_beam_search_decode(lm, 100)
  text_out = [''.join(' ' if i == 27 else LETTERS[i] for i in s) for s in ids[:2]]
  n_words = [len(s.split()) for s in text_out]
  rec = {'workload': 'configs[4] shard: batch {} x T\'={}, input log10(softmax + 1e-8)'.format(B, T),
         'model': dict(lm.info, synthetic_seed=1234),
         'ms_device': {k: round(v, 3) for k, v in med.items()},
         'ms_device_all': {k: [round(x, 3) for x in v] for k, v in ms.items()},
         'lm_over_lm_free_beam100': round(med['lm_beam100'] / med['lm_free_beam100'], 3),
         'lm_load_s': {'generate_text': round(t_gen, 2), 'parse_and_tables': round(t_parse, 2), 'upload': round(t_upload, 3)},
         'lm_weights': {'lm_weight': 0.8, 'word_count_weight': 0.0, 'valid_word_count_weight': 2.3, 'oov_score': -1000.0},
         'decoded_words_rows_0_1': n_words,
         'method': 'median of {} samples, each the mean of {} back-to-back calls between HIP events (log-softmax rows + search '
                   'kernel), variants alternated'.format(args.samples, args.reps),
         'device': torch.cuda.get_device_name(0)}
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(rec, f, indent=1)
  print(json.dumps(rec))


if __name__ == '__main__':
  main()
