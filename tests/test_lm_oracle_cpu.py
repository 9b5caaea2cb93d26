"""The float64 specification of the LM-scored beam search (tests/lm_oracle.py) pinned independently of itself: with every
weight 0 it IS the LM-free recursion, and with an unbounded beam its top path is the exhaustive argmax of
ln p_ctc(P) + lm_weight * LM(P)."""
import itertools
import math
import os

import numpy as np
import pytest

from tests import lm_oracle as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, 'tests', 'golden', 'lm_tiny.arpa')


def word_logits(text, rng, frames_per_char=3, gap=1, noise=1.0, peak=5.0):
  """[T, 29] logits that spell `text`: each character peaks for a few frames, a blank frame between characters."""
  rows = []
  for ch in text:
    c = L.SPACE if ch == ' ' else L.LETTERS.index(ch)
    for _ in range(frames_per_char):
      r = rng.standard_normal(29) * noise
      r[c] += peak
      rows.append(r)
    for _ in range(gap):
      r = rng.standard_normal(29) * noise
      r[28] += peak
      rows.append(r)
  return np.array(rows)


@pytest.mark.parametrize('transform', [None, 'log10_softmax'])
def test_zero_weights_equal_the_lm_free_search(transform):
  lm = L.ArpaModel.load(TINY)
  rng = np.random.default_rng(3)
  T, B = 40, 3
  logits = rng.standard_normal((T, B, 29)) * 2.0
  w = word_logits('on the mat', rng, frames_per_char=2, gap=1)
  logits[:len(w), 1, :] = w
  lens = [40, len(w), 0]
  for beam in (1, 8, 30):
    ids, score = L.lm_beam_search_decode(logits, lens, lm, beam, transform, lm_weight=0.0, word_count_weight=0.0,
                                         valid_word_count_weight=0.0)
    ref_ids, ref_score = L.lm_free_equivalent(logits, lens, beam, transform)
    assert ids == ref_ids
    assert np.array_equal(score, ref_score)


@pytest.mark.parametrize('seed,weights', [(0, (0.8, 0.0, 2.3)), (1, (1.5, -0.5, 1.0)), (2, (0.3, 1.0, 0.0))])
def test_unbounded_beam_equals_exhaustive_enumeration(seed, weights):
  lm = L.ArpaModel.load(TINY)
  lw, wcw, vwcw = weights
  rng = np.random.default_rng(seed)
  T = 3
  x = rng.standard_normal((T, 29)) * 1.5
  x[:, [2, 0, 19, 27, 28]] += 2.0                 # c, a, t, space, blank: LM-relevant prefixes near the top
  lp = x - x.max(axis=1, keepdims=True)
  lp = lp - np.log(np.exp(lp).sum(axis=1, keepdims=True))
  # every labelling of length <= 3 and its ln p_ctc, by summing over all 29^3 alignments once
  probs = {}
  for path in itertools.product(range(29), repeat=T):
    out, prev = [], None
    for c in path:
      if c != 28 and c != prev:
        out.append(c)
      prev = c
    key = tuple(out)
    probs[key] = np.logaddexp(probs.get(key, -math.inf), sum(lp[t, c] for t, c in enumerate(path)))
  sc = L.Scorer(lm, wcw, vwcw)
  best_key, best = None, -math.inf
  for key, p in probs.items():
    v = p + lw * (sc.state(key)[3] + sc.end_delta(key))
    if v > best:
      best_key, best = key, v
  ids, score = L.lm_beam_search_decode(x[:, None, :], [T], lm, beam_width=100000, lm_weight=lw, word_count_weight=wcw,
                                       valid_word_count_weight=vwcw)
  assert tuple(ids[0]) == best_key
  assert score[0, 0] == pytest.approx(best, abs=1e-9)


def test_spelling_is_decided_by_the_language_model():
  lm = L.ArpaModel.load(TINY)
  rng = np.random.default_rng(7)
  x = word_logits('the kat', rng, noise=0.3)
  # acoustics slightly favour k over c in the third word
  k, c = L.LETTERS.index('k'), L.LETTERS.index('c')
  for t in range(len(x)):
    if x[t].argmax() == k:
      x[t, c] = x[t, k] - 0.5
  plain, _ = L.lm_free_equivalent(x[:, None, :], [len(x)], 16)
  assert L.ids_to_text(plain[0]) == 'the kat'
  ids, _ = L.lm_beam_search_decode(x[:, None, :], [len(x)], lm, beam_width=16)
  assert L.ids_to_text(ids[0]) == 'the cat'
