"""N-best lists of the CTC beam searches and their second-pass rescoring.

`engine.beam_search_decode_nbest` / `engine.lm_beam_search_decode_nbest` return, per utterance, the N best final prefixes of the
search as (ids, log_prob).  In the LM search the LM state is a function of the prefix alone, so a hypothesis' score splits exactly:

  log_prob = acoustic + lm_weight * (G + word_count_weight * n_words + valid_word_count_weight * n_valid)

with G the sum of the log10 n-gram probabilities of the prefix's words plus </s>, n_words / n_valid counts, and `acoustic` the
beam's acoustic mass for the prefix.  G and the counts depend on the prefix and the model only (`engine.lm_score_prefixes`, a
kernel with a bit-identical host form), so a list can be re-ranked under other weights, or under another model that could not
run inside the search, without searching again: `components` splits the first pass, `rescore` re-ranks.
"""
import numpy as np


class Hypothesis(dict):
  """One entry of an N-best list: {'ids', 'log_prob'} and, after `components`, {'acoustic', 'lm_log10', 'words', 'valid_words'}
  (the last three only when a model was involved) and 'bias' (only when the first pass had hotwords)."""


def as_lists(lists):
  """[(ids, log_prob), ...] per utterance (what the engine returns) -> lists of Hypothesis, rank order kept."""
  return [[h if isinstance(h, dict) else Hypothesis(ids=list(h[0]), log_prob=float(h[1])) for h in hyps] for hyps in lists]


def _scores(engine, lm, lists):
  """(G, n_words, n_valid) of every hypothesis of every list, in one call, back in the lists' shape."""
  flat = [h['ids'] for hyps in lists for h in hyps]
  g, n_words, n_valid = engine.lm_score_prefixes(lm, flat)
  out, k = [], 0
  for hyps in lists:
    out.append([(float(g[k + i]), int(n_words[k + i]), int(n_valid[k + i])) for i in range(len(hyps))])
    k += len(hyps)
  return out


def components(engine, lm, lists, first_pass_weights=None, hotwords=None):
  """Attaches to each hypothesis of ``lists`` (per utterance [(ids, log_prob), ...] or Hypothesis dicts) its parts under the
  first pass: ``lm_log10`` = G, ``words``, ``valid_words`` under ``lm``, and ``acoustic`` = log_prob - lm_weight * (G +
  word_count_weight * words + valid_word_count_weight * valid_words), computed in double, with ``first_pass_weights`` =
  (lm_weight, word_count_weight, valid_word_count_weight) of the search that made the lists.  ``lm=None`` (an LM-free first
  pass): ``acoustic`` = log_prob and nothing else is attached.  ``hotwords`` (the `hotwords.Hotwords` of a biased first pass): each
  hypothesis also gets ``bias``, its final hotword credit with the weight included, and ``acoustic`` is without it -- so that rescoring
  under a second model keeps the first pass's bias out of the acoustic part.  Returns the lists as Hypothesis dicts."""
  lists = as_lists(lists)
  bias = (lambda h: float(hotwords.score(h['ids'])[1])) if hotwords is not None else (lambda h: 0.0)
  if lm is None:
    for hyps in lists:
      for h in hyps:
        h['acoustic'] = float(h['log_prob']) - bias(h)
  else:
    lw, wc, vwc = (float(x) for x in first_pass_weights)
    for hyps, parts in zip(lists, _scores(engine, lm, lists)):
      for h, (g, n_words, n_valid) in zip(hyps, parts):
        h.update(lm_log10=g, words=n_words, valid_words=n_valid,
                 acoustic=float(h['log_prob']) - lw * (g + wc * n_words + vwc * n_valid) - bias(h))
  if hotwords is not None:
    for hyps in lists:
      for h in hyps:
        h['bias'] = bias(h)
  return lists


def rerank(scores):
  """Order of a list under new scores: best first, ties to the lower first-pass rank."""
  return sorted(range(len(scores)), key=lambda i: (-scores[i], i))


def _rescore(lists, engine, lm2, lm_weight, word_count_weight, valid_word_count_weight):
  lw, wc, vwc = float(lm_weight), float(word_count_weight), float(valid_word_count_weight)
  all_parts = _scores(engine, lm2, lists)
  orders, new_scores = [], []
  for hyps, parts in zip(lists, all_parts):
    s = [float(h['acoustic']) + lw * (g + wc * n_words + vwc * n_valid) for h, (g, n_words, n_valid) in zip(hyps, parts)]
    order = rerank(s)
    orders.append(order)
    new_scores.append(np.array([s[i] for i in order], dtype=np.float64))
  return orders, new_scores, all_parts


def rescore(lists, engine, lm2, lm_weight, word_count_weight=0.0, valid_word_count_weight=0.0):
  """Re-ranks each list (hypotheses with ``acoustic``, see `components`) under ``lm2``: the score of a hypothesis is
  acoustic + lm_weight * (G2 + word_count_weight * n_words + valid_word_count_weight * n_valid) with G2 and the counts taken
  from ``lm2``; ties go to the lower first-pass rank.
  -> (order, scores): per utterance the first-pass ranks in their new order, and the new scores in that order (float64)."""
  return _rescore(lists, engine, lm2, lm_weight, word_count_weight, valid_word_count_weight)[:2]


def rescored(lists, engine, lm2, lm_weight, word_count_weight=0.0, valid_word_count_weight=0.0):
  """`rescore`, applied: the lists in their new order, each hypothesis with ``log_prob`` = its new score, ``lm_log10`` / ``words`` /
  ``valid_words`` under ``lm2``, its ``acoustic`` unchanged, and ``first_pass_rank`` / ``first_pass_log_prob``."""
  orders, scores, parts = _rescore(lists, engine, lm2, lm_weight, word_count_weight, valid_word_count_weight)
  out = []
  for hyps, order, new, part in zip(lists, orders, scores, parts):
    out.append([Hypothesis(hyps[i], log_prob=float(v), lm_log10=part[i][0], words=part[i][1], valid_words=part[i][2],
                           first_pass_rank=i, first_pass_log_prob=float(hyps[i]['log_prob'])) for i, v in zip(order, new)])
  return out
