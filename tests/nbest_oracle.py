"""N-best lists of the two CTC prefix beam searches and their second-pass rescoring: the float64 specification.

The searches are those of ``oracle/w2l_oracle.py::ctc_beam_search_decode`` and ``tests/lm_oracle.py::lm_beam_search_decode``,
restated here so that they return the whole ranked final set instead of its top path (tests/test_nbest_cpu.py pins the first
hypothesis and its score to those two).  Ranking rules (include/speecht_hip.h):

  - LM-free: the hypotheses are the entries of the final set in its own order -- (total desc, candidate key asc);
  - LM: every entry first gains ``lm_weight *`` its end-of-utterance delta (the incomplete word, then ``</s>``); the entries are then
    ranked by (final total desc, rank in the set asc);
  - a list holds min(n_best, entries alive) hypotheses: an utterance of length 0 has one, the empty prefix.

The LM state is a function of the prefix alone and every inflow into a prefix carries the same ``lm_weight * delta``, so a final
total splits exactly as

  total = A + lm_weight * (G + word_count_weight * n_words + valid_word_count_weight * n_valid)

with A the beam's acoustic mass for the prefix and (G, n_words, n_valid) = ``sentence_score`` below, which depends on the prefix and
the model only (``oov_score`` never enters: a completed out-of-vocabulary word is scored as ``<unk>``).  ``rescore`` re-ranks a
list under other weights or another model from A alone.

``dtype=np.float32`` runs the recursion's arithmetic in float32 (the LM terms still come from the float64 scorer, rounded): the
tests use it to show that the sets they compare do not hinge on the precision of the search.
"""
import math

import numpy as np

from tests import lm_oracle as L

SPACE = L.SPACE


def sentence_score(lm, prefix):
  """(G, n_words, n_valid) of a prefix (ids 0..27) under an ``lm_oracle.ArpaModel``: the ids are cut at every space into words; an
  empty run (a leading space, two spaces in a row) counts as a word and scores as <unk>; the trailing run counts only if it is
  non-empty.  The context starts as <s> (order > 1) and keeps the last order - 1 words.  A word spelled in [a-z'] that is a unigram
  scores as itself and counts in n_valid, any other as <unk>.  G = sum of log10 p(word | ctx) + log10 p(</s> | ctx), float32 table
  values summed in double in word order, </s> last."""
  words, run = [], []
  for c in prefix:
    c = int(c)
    if not 0 <= c <= SPACE:
      raise ValueError('id {} outside 0..27'.format(c))
    if c == SPACE:
      words.append(''.join(run))
      run = []
    else:
      run.append(L.LETTERS[c])
  if run:
    words.append(''.join(run))
  ctx = ('<s>',)[:max(lm.order - 1, 0)]
  g, n_valid = 0.0, 0
  for word in words:
    valid = word in lm.vocab
    w = word if valid else '<unk>'
    g += lm.logp(ctx, w)
    n_valid += int(valid)
    ctx = (ctx + (w,))[max(0, len(ctx) + 1 - (lm.order - 1)):]
  g += lm.logp(ctx, '</s>')
  return g, len(words), n_valid


def _rows(logits_tm, input_transform, dtype):
  x = L._transform(logits_tm, input_transform)                    # float64, as the searches this restates
  lp = np.empty_like(x)
  for t in range(x.shape[0]):
    for b in range(x.shape[1]):                                   # row by row, the very operations of the searches restated
      row = x[t, b] - x[t, b].max()
      lp[t, b] = row - math.log(np.exp(row).sum())
  return lp.astype(dtype)


def final_sets(logits_tm, seq_lens, beam_width, input_transform=None, lm=None, lm_weight=0.8, word_count_weight=0.0,
               valid_word_count_weight=2.3, oov_score=-1000.0, dtype=np.float64):
  """The ranked final set of every utterance: a list (per utterance) of (prefix tuple, total, acoustic part), best first.
  ``lm=None``: the LM-free search, total = acoustic part = lse(p_blank, p_label).  With a model: total = lse(p_blank, p_label) +
  lm_weight * end_delta(prefix); the acoustic part is the lse of a second pair (p_blank, p_label) that the same search carries
  through the same entries by the same recursion without the LM deltas -- the beam's acoustic mass A of the prefix."""
  T, B, C = np.shape(logits_tm)
  if lm is not None:
    assert C == SPACE + 2, 'classes a-z \' space blank'
  lp_all = _rows(logits_tm, input_transform, dtype)
  f = dtype
  blank, ninf = C - 1, f(-np.inf)
  lse = lambda a, b: f(np.logaddexp(f(a), f(b)))
  lw = f(lm_weight)
  out = []
  for b in range(B):
    sc = L.Scorer(lm, word_count_weight, valid_word_count_weight, oov_score) if lm is not None else None
    beams = [((), f(0.0), ninf, f(0.0), ninf)]           # (prefix, p_blank, p_label, acoustic p_blank, acoustic p_label)
    for t in range(min(int(seq_lens[b]), T)):
      lp = lp_all[t, b]
      slot_of = {e[0]: i for i, e in enumerate(beams)}
      cands = []
      for slot, (pre, pb, pl, apb, apl) in enumerate(beams):
        tot, atot = lse(pb, pl), lse(apb, apl)
        stay_b, astay_b = f(tot + lp[blank]), f(atot + lp[blank])
        stay_l = astay_l = ninf
        if pre:
          mass, amass = pl, apl
          if pre[:-1] in slot_of:
            ppre, ppb, ppl, papb, papl = beams[slot_of[pre[:-1]]]
            repeat = bool(ppre) and ppre[-1] == pre[-1]
            inflow = ppb if repeat else lse(ppb, ppl)
            mass = lse(mass, f(inflow + lw * f(sc.delta(pre))) if sc is not None else inflow)
            amass = lse(amass, papb if repeat else lse(papb, papl))
          stay_l, astay_l = f(mass + lp[pre[-1]]), f(amass + lp[pre[-1]])
        cands.append((lse(stay_b, stay_l), slot * C + blank, pre, stay_b, stay_l, astay_b, astay_l))
        for c in range(C - 1):
          child = pre + (c,)
          if child in slot_of:
            continue
          repeat = bool(pre) and pre[-1] == c
          base = pb if repeat else tot
          v = f(lp[c] + f(base + lw * f(sc.delta(child)))) if sc is not None else f(base + lp[c])
          cands.append((v, slot * C + c, child, ninf, v, ninf, f((apb if repeat else atot) + lp[c])))
      cands = [x for x in cands if x[0] > ninf]
      cands.sort(key=lambda x: (-x[0], x[1]))
      beams = [x[2:] for x in cands[:beam_width]]
    entries = []
    for rank, (pre, pb, pl, apb, apl) in enumerate(beams):
      total = lse(pb, pl)
      if sc is not None:
        total = f(total + lw * f(sc.end_delta(pre)))
      entries.append((pre, float(total), float(lse(apb, apl)), rank))
    if sc is not None:
      entries.sort(key=lambda e: (-e[1], e[3]))
    out.append([(pre, total, a) for pre, total, a, _ in entries])
  return out


def nbest(logits_tm, seq_lens, n_best, beam_width, **kw):
  """The N-best lists: per utterance [(id list, score), ...] -- the first min(n_best, entries alive) of `final_sets`."""
  return [[(list(pre), total) for pre, total, _ in entries[:n_best]] for entries in final_sets(logits_tm, seq_lens, beam_width, **kw)]


def rerank(scores):
  """Best first; ties go to the lower first-pass rank."""
  return sorted(range(len(scores)), key=lambda i: (-scores[i], i))


def split(lm, hyps, lm_weight, word_count_weight, valid_word_count_weight):
  """[(ids, score)] of an LM search -> [(ids, acoustic)]: acoustic = score - lm_weight * (G + wc * n_words + vwc * n_valid)."""
  out = []
  for ids, score in hyps:
    g, nw, nv = sentence_score(lm, ids)
    out.append((ids, score - lm_weight * (g + word_count_weight * nw + valid_word_count_weight * nv)))
  return out


def rescore(hyps, lm2, lm_weight, word_count_weight=0.0, valid_word_count_weight=0.0):
  """[(ids, acoustic)] in first-pass order -> (order, scores): the first-pass ranks in their new order under
  acoustic + lm_weight * (G2 + wc * n_words + vwc * n_valid) with (G2, n_words, n_valid) from ``lm2``, and the scores in that order."""
  s = []
  for ids, acoustic in hyps:
    g, nw, nv = sentence_score(lm2, ids)
    s.append(acoustic + lm_weight * (g + word_count_weight * nw + valid_word_count_weight * nv))
  order = rerank(s)
  return order, [s[i] for i in order]


def near_tie_share(scores, n, tau):
  """(pairs within tau, pairs) among the adjacent pairs of the first n + 1 scores of a ranked list."""
  head = scores[:n + 1]
  gaps = [head[i] - head[i + 1] for i in range(len(head) - 1)]
  return sum(1 for g in gaps if g <= tau), len(gaps)


TAU = 1e-4        # the figure the kernel's own lse comment and the existing beam-search tests hold scores to


def check_list(got, entries, n_best, tau=TAU, tol=1e-4):
  """A device list ``got`` = [(ids, score), ...] against the oracle's ranked final set ``entries`` (of `final_sets`):
  (a) the number of hypotheses is exact; (b) every returned prefix is in the oracle's final set with the oracle's score for it
  (rtol = atol = tol), and the returned scores do not increase; (c) order and membership are exact except among near ties: a pair
  the list orders differently from the oracle has oracle scores within tau, and an oracle hypothesis missing from the list lies
  within tau of the oracle's (n + 1)-th score -- and a member of the list from beyond the oracle's first n within tau of its n-th.  Raises AssertionError with the offending figures."""
  n = min(n_best, len(entries))
  assert len(got) == n, ('n_hyps', len(got), n)
  score_of = {pre: total for pre, total, _ in entries}
  rank_of = {pre: r for r, (pre, _, _) in enumerate(entries)}
  keys = [tuple(ids) for ids, _ in got]
  assert len(set(keys)) == len(keys), 'a prefix twice'
  for (ids, s), key in zip(got, keys):
    assert key in score_of, ('not in the final set', ids)
    ref = score_of[key]
    assert abs(s - ref) <= tol + tol * abs(ref), ('score', ids, s, ref)
  scores = [s for _, s in got]
  assert all(a >= b for a, b in zip(scores, scores[1:])), ('scores increase', scores)
  for i in range(len(keys)):
    for j in range(i + 1, len(keys)):
      if rank_of[keys[i]] > rank_of[keys[j]]:
        gap = abs(score_of[keys[i]] - score_of[keys[j]])
        assert gap <= tau, ('order', keys[i], keys[j], gap)
  for key in keys:
    if rank_of[key] >= n:
      assert entries[n - 1][1] - score_of[key] <= tau, ('from beyond the first n', key, score_of[key])
  have = set(keys)
  for pre, total, _ in entries[:n]:
    if pre not in have:
      assert len(entries) > n and total - entries[n][1] <= tau, ('missing', pre, total)
