"""Hotword biasing of the two CTC prefix beam searches: the float64 specification, in plain Python.

Input: K phrases, each a string of 1..64 ids in 0..27 (a-z, apostrophe, space), and one weight w >= 0 per matched character.  A
hypothesis with prefix x scores, during the search,

  total(x) = CTC mass + lm_weight * LM terms (if a model is loaded) + w * (M(x) + r(x))

and at the end of the utterance ``w * r(x)`` is replaced by what the flush rule banks.  M is the number of characters of completed
phrase occurrences banked so far, r the length of the partial match still open: a partial match earns credit while it grows and
gives it back when it fails.

The scan (`Scan`): x is read left to right with a state, the open partial match -- a string that is a prefix of some phrase (a node
of the phrases' trie; `Scan` keeps the string itself).

  - on label c, (a): if open + c is a prefix of a phrase, move to it; if it IS a phrase and no longer phrase continues it, bank its
    length and return to the root;
  - on label c, (b), otherwise: at the root, stay.  Else let t be the longest phrase that is a prefix of the open match (the match
    itself included); bank len(t) (0 without one); take u = the open match without its first len(t) characters, or without its first
    character if there is no t; restart at the root and feed u, then c, by these same rules;
  - end of utterance (flush): repeat the resolution of (b) without a new label until the state is the root; what is banked on the way
    counts, the rest is forfeited;
  - a label outside 0..27 (an LM-free search may have further classes) neither advances nor breaks a match.

Both rules are pure functions of (state, c) and of the state, so they tabulate (`tables`): with the states numbered breadth first --
the prefixes of the phrases sorted by (length, ids), the root 0 --

  next[n][c];  gain[n][c] = w * (banked + depth(next) - depth(n));  fin[n] = w * (flush bank - depth(n))

as int32 [N][32], float32 [N][32] (columns >= 28: the state itself, 0) and float32 [N].

`final_sets` restates ``nbest_oracle.final_sets`` with the extra term: the gain of the prefix's last label goes wherever the LM's
``delta`` goes (child candidates, the stay candidate's parent inflow) and ``fin`` wherever ``end_delta`` goes, with or without a model;
the final set is then ranked by (final total desc, rank in the set asc) in both searches.
"""
import numpy as np

from tests import lm_oracle as L
from tests import nbest_oracle as N

LABELS = 28
PITCH = 32
MAX_PHRASE = 64


def as_phrases(phrases):
  """Strings or id lists -> tuples of ids, duplicates dropped in order."""
  out = []
  for p in phrases:
    ids = tuple(L.words_to_ids(p.lower())) if isinstance(p, str) else tuple(int(i) for i in p)
    assert 1 <= len(ids) <= MAX_PHRASE and all(0 <= i < LABELS for i in ids), p
    if ids not in out:
      out.append(ids)
  return out


class Scan:
  """The rules on strings: the definition."""

  def __init__(self, phrases):
    self.phrases = set(as_phrases(phrases))
    self.paths = {p[:k] for p in self.phrases for k in range(len(p) + 1)} | {()}
    self.inner = {p[:-1] for p in self.paths if p}               # paths that some longer path continues

  def resolve(self, match):
    """(b) without the label: (banked, u) of a non-empty open match."""
    t = max((k for k in range(1, len(match) + 1) if match[:k] in self.phrases), default=0)
    return t, (match[t:] if t else match[1:])

  def step(self, match, c):
    """-> (the open match after label c, characters banked by it)."""
    c = int(c)
    if not 0 <= c < LABELS:
      return match, 0
    longer = match + (c,)
    if longer in self.paths:
      if longer in self.phrases and longer not in self.inner:
        return (), len(longer)
      return longer, 0
    if not match:
      return (), 0
    bank, u = self.resolve(match)
    match = ()
    for ch in u + (c,):
      match, b = self.step(match, ch)
      bank += b
    return match, bank

  def flush(self, match):
    """-> characters banked at the end of the utterance from an open match."""
    bank = 0
    while match:
      b, u = self.resolve(match)
      bank += b
      match = ()
      for ch in u:
        match, b = self.step(match, ch)
        bank += b
    return bank

  def scan(self, x):
    """-> ([(M, r) after every label of x], M at the end of the utterance)."""
    match, m, out = (), 0, []
    for c in x:
      match, b = self.step(match, c)
      m += b
      out.append((m, len(match)))
    return out, m + self.flush(match)


def scores(phrases, weight, x):
  """-> (the bias of every non-empty prefix of x during the search, the final bias of x), float64."""
  during, m = Scan(phrases).scan(x)
  return [weight * (a + r) for a, r in during], weight * m


def states(phrases):
  """The trie's nodes as strings, breadth first: sorted by (length, ids)."""
  return sorted(Scan(phrases).paths, key=lambda p: (len(p), p))


def tables(phrases, weight=1.0):
  """-> (next int32 [N][32], gain float32 [N][32], fin float32 [N]) from the rules on strings, state by state and label by label."""
  sc = Scan(phrases)
  nodes = states(phrases)
  index = {p: i for i, p in enumerate(nodes)}
  nxt = np.zeros((len(nodes), PITCH), np.int32)
  gain = np.zeros((len(nodes), PITCH), np.float32)
  fin = np.zeros(len(nodes), np.float32)
  for i, p in enumerate(nodes):
    nxt[i, :] = i
    for c in range(LABELS):
      q, bank = sc.step(p, c)
      nxt[i, c] = index[q]
      gain[i, c] = float(weight) * (bank + len(q) - len(p))
    fin[i] = float(weight) * (sc.flush(p) - len(p))
  return nxt, gain, fin


def table_scan(tabs, x):
  """The bias along x from the tables alone -> (during [len(x)], final), float64 sums of the table values."""
  nxt, gain, fin = tabs
  n, s, out = 0, 0.0, []
  for c in x:
    s += float(gain[n, c])
    n = int(nxt[n, c])
    out.append(s)
  return out, s + float(fin[n])


class Bias:
  """The second scorer of the searches: `delta` / `end_delta` of a prefix, like ``lm_oracle.Scorer`` (state cached by prefix)."""

  def __init__(self, phrases, weight):
    self.sc, self.w = Scan(phrases), float(weight)
    self.open = {(): ()}

  def state(self, prefix):
    st = self.open.get(prefix)
    if st is None:
      st = self.open[prefix] = self.sc.step(self.state(prefix[:-1]), prefix[-1])[0]
    return st

  def delta(self, prefix):
    before = self.state(prefix[:-1])
    after, bank = self.sc.step(before, prefix[-1])
    return self.w * (bank + len(after) - len(before))

  def end_delta(self, prefix):
    match = self.state(prefix)
    return self.w * (self.sc.flush(match) - len(match))


def final_sets(logits_tm, seq_lens, beam_width, input_transform=None, lm=None, lm_weight=0.8, word_count_weight=0.0,
               valid_word_count_weight=2.3, oov_score=-1000.0, dtype=np.float64, hotwords=(), hotword_weight=1.0):
  """``nbest_oracle.final_sets`` with hotwords: the ranked final set of every utterance as (prefix tuple, total, acoustic part),
  best first; total = acoustic mass + lm_weight * LM terms + the prefix's final bias.  Without phrases, or with weight 0, the result
  is that of ``nbest_oracle.final_sets``."""
  T, B, C = np.shape(logits_tm)
  if lm is not None:
    assert C == N.SPACE + 2, 'classes a-z \' space blank'
  lp_all = N._rows(logits_tm, input_transform, dtype)
  f = dtype
  blank, ninf = C - 1, f(-np.inf)
  lse = lambda a, b: f(np.logaddexp(f(a), f(b)))
  lw = f(lm_weight)
  out = []
  for b in range(B):
    sc = L.Scorer(lm, word_count_weight, valid_word_count_weight, oov_score) if lm is not None else None
    hot = Bias(hotwords, hotword_weight)

    def entered(base, prefix):
      """The mass that flows into `prefix` from its parent's `base`: the LM delta, then the hotword gain."""
      if sc is not None:
        base = f(base + lw * f(sc.delta(prefix)))
      return f(base + f(hot.delta(prefix)))

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
            mass = lse(mass, entered(ppb if repeat else lse(ppb, ppl), pre))
            amass = lse(amass, papb if repeat else lse(papb, papl))
          stay_l, astay_l = f(mass + lp[pre[-1]]), f(amass + lp[pre[-1]])
        cands.append((lse(stay_b, stay_l), slot * C + blank, pre, stay_b, stay_l, astay_b, astay_l))
        for c in range(C - 1):
          child = pre + (c,)
          if child in slot_of:
            continue
          repeat = bool(pre) and pre[-1] == c
          v = f(lp[c] + entered(pb if repeat else tot, child))
          cands.append((v, slot * C + c, child, ninf, v, ninf, f((apb if repeat else atot) + lp[c])))
      cands = [x for x in cands if x[0] > ninf]
      cands.sort(key=lambda x: (-x[0], x[1]))
      beams = [x[2:] for x in cands[:beam_width]]
    entries = []
    for rank, (pre, pb, pl, apb, apl) in enumerate(beams):
      total = lse(pb, pl)
      if sc is not None:
        total = f(total + lw * f(sc.end_delta(pre)))
      total = f(total + f(hot.end_delta(pre)))
      entries.append((pre, float(total), float(lse(apb, apl)), rank))
    entries.sort(key=lambda e: (-e[1], e[3]))
    out.append([(pre, total, a) for pre, total, a, _ in entries])
  return out
