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


class ArenaError(ValueError):
  """The arena of a streaming N-best read-out does not hold what the device writes (`read_arena`)."""


ARENA_HEADER = 6


def read_arena(arena, used, prefixes, skip=()):
  """The records st_ctc_beam_stream_read_nbest / _step_pieces_nbest left (include/speecht_hip.h) -> ``(lists, lost)``.
  ``arena``: the int32 words of the arena (all of them or the first ``used``: its length is taken for the capacity when ``used`` is
  larger); ``used``: the call's counter, the words all finishing read-outs asked for; ``prefixes``: {(piece, stream): ids} for every
  final the call may have closed -- the labels the host holds for that stream, at least the record's old stable length of them (the
  device stores a hypothesis from there on).  ``lists``: {(piece, stream): [Hypothesis(ids, log_prob), ...]}, best first, whatever
  order the records arrived in.  ``lost``: the words asked for beyond the records that fit -- 0 unless ``used`` exceeds the capacity;
  what lies behind the last whole record is then not read (the device wrote nothing there), and the caller finds the lost lists by
  their keys.  With ``used`` inside the capacity every word must belong to a well-formed record of a key in ``prefixes``, each at most
  once: anything else raises `ArenaError`, and no index ever leaves ``arena[:used]``.  ``skip``: keys whose records exist but are not
  wanted -- the device writes a finishing read-out's record whatever the host then makes of that read-out (a search whose status says
  it gave up, a tail longer than the host can take) -- such a record must be well formed, is stepped over and yields no list."""
  arena = np.ascontiguousarray(np.asarray(arena, dtype=np.int32).reshape(-1))
  used = int(used)
  if used < 0:
    raise ArenaError('the arena\'s counter is negative ({})'.format(used))
  over = used > len(arena)
  end = min(used, len(arena))
  lists, skipped, pos = {}, set(), 0
  while pos < end:
    bad, rec = None, arena[pos:pos + ARENA_HEADER].tolist()
    if len(rec) < ARENA_HEADER or pos + ARENA_HEADER > end:
      bad = 'a header at word {} runs past the {} words used'.format(pos, end)
    else:
      stream, piece, n, old, words, zero = rec
      key = (piece, stream)
      if zero != 0 or n < 1 or stream < 0 or piece < 0 or old < 0 or words < ARENA_HEADER + 2 * n:
        bad = 'the header at word {} is malformed: {}'.format(pos, rec)
      elif pos + words > end:
        bad = 'the record at word {} has {} words, {} are used'.format(pos, words, end)
      elif key in lists or key in skipped:
        bad = 'a second record for piece {} of stream {} at word {}'.format(piece, stream, pos)
      elif key not in skip and (key not in prefixes or len(prefixes[key]) < old):
        bad = 'the record at word {} (piece {}, stream {}, {} stable labels) is none the caller expects'.format(pos, piece, stream, old)
      else:
        pairs = arena[pos + ARENA_HEADER:pos + ARENA_HEADER + 2 * n].reshape(n, 2)
        tails = pairs[:, 0].astype(np.int64) - old
        if (tails < 0).any() or int(tails.sum()) != words - ARENA_HEADER - 2 * n:
          bad = 'the record at word {}: its lengths {} above {} stable labels do not fill {} words'.format(
              pos, pairs[:, 0].tolist(), old, words)
    if bad is not None:
      if over:                                                   # behind the records that fit: not the device's words
        break
      raise ArenaError(bad)
    if key in skip:
      skipped.add(key)
      pos += words
      continue
    head = list(prefixes[key][:old])
    ends = pos + ARENA_HEADER + 2 * n + np.cumsum(tails)
    log_probs = np.ascontiguousarray(pairs[:, 1]).view(np.float32)
    lists[key] = [Hypothesis(ids=head + arena[e - t:e].tolist(), log_prob=float(lp))
                  for e, t, lp in zip(ends.tolist(), tails.tolist(), log_probs)]
    pos += words
  return lists, used - pos


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
  under a second model keeps the first pass's bias out of the acoustic part.  A list or tuple of ``hotwords`` names one per list (None:
  that list's search was not biased) -- the finals of live streams with a phrase set each, their model scores still taken in one call.
  Returns the lists as Hypothesis dicts."""
  lists = as_lists(lists)
  per_list = list(hotwords) if isinstance(hotwords, (list, tuple)) else [hotwords] * len(lists)
  if len(per_list) != len(lists):
    raise ValueError('components: {} hotword sets for {} lists'.format(len(per_list), len(lists)))
  score = lambda hot: (lambda h: float(hot.score(h['ids'])[1])) if hot is not None else (lambda h: 0.0)
  if lm is None:
    for hyps, hot in zip(lists, per_list):
      bias = score(hot)
      for h in hyps:
        h['acoustic'] = float(h['log_prob']) - bias(h)
  else:
    lw, wc, vwc = (float(x) for x in first_pass_weights)
    for hyps, parts, hot in zip(lists, _scores(engine, lm, lists), per_list):
      bias = score(hot)
      for h, (g, n_words, n_valid) in zip(hyps, parts):
        h.update(lm_log10=g, words=n_words, valid_words=n_valid,
                 acoustic=float(h['log_prob']) - lw * (g + wc * n_words + vwc * n_valid) - bias(h))
  for hyps, hot in zip(lists, per_list):
    if hot is not None:
      bias = score(hot)
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
