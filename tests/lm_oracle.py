"""LM-scored CTC prefix beam search: the specification of the word n-gram scorer, restated in float64.

It extends the recursion of ``oracle/w2l_oracle.py::ctc_beam_search_decode`` (stock ``tf.nn.ctc_beam_search_decoder``, top path,
candidates ranked by (total desc, slot*C + c asc)) with the scorer hooks of TF's ``ctc_beam_search.h`` -- ``ExpandState``,
``GetStateExpansionScore``, ``ExpandStateEnd`` / ``GetStateEndExpansionScore`` -- filled in with a word n-gram model read from
an ARPA file.  With every weight 0 it returns exactly what ``ctc_beam_search_decode`` returns (tests/test_lm_oracle_cpu.py).

PARITY UNPINNED: the reference runs this decoder through its KenLM TensorFlow fork (speech_model.py:84-111), which is not
vendored; nothing here was compared against a run of it.  Two choices were reconstructed from the fork's published design rather
than read from its source: an incomplete word is scored by the LOWEST unigram log10 probability among the vocabulary words it
is a prefix of, and a prefix that has left the vocabulary scores ``oov_score`` (-1000).

The LM state of a beam entry (a function of its prefix alone):
  - ``ctx``: the last N-1 words (N = the ARPA order); the root's context is ``<s>``;
  - the incomplete word (the letters since the last space) and whether it is still a prefix of a vocabulary word;
  - ``lm_score``: the scores of the words completed so far, bonuses included;
  - ``score`` = lm_score + the incomplete word's lowest completion unigram (0 at a word start, oov_score off the vocabulary).
Expanding with a letter (ids 0..26: a-z, ') extends the incomplete word; expanding with space (27) scores the incomplete word
against ``ctx`` with ARPA backoff -- ``<unk>`` if it is not a vocabulary word, the empty word included -- adds
``word_count_weight`` and, for a vocabulary word, ``valid_word_count_weight``, shifts the word into ``ctx`` and starts a new word.
``delta`` = score - the parent's score; ``lm_weight * delta`` is added to every transition into a prefix: the child candidate
``input(c) + lm_weight*delta(child) + previous`` and the parent inflow of the stay candidate ``lse(p_label, previous +
lm_weight*delta(self))``.  At the end every surviving entry scores its incomplete word (if non-empty) and ``</s>``; its total
gains ``lm_weight *`` that delta, and the top path is the best total after it (ties: the lower rank); ``log_prob`` includes
the LM terms.

ARPA values are read as float32 (what the device tables hold) and computed with in float64.  Words are lowercased; words
spelled outside [a-z'] keep their n-grams but can never be spelled by the decoder.
"""
import gzip
import math

import numpy as np

from oracle import w2l_oracle as O

SPACE = 27
LETTERS = "abcdefghijklmnopqrstuvwxyz'"


def _f32(text):
  return float(np.float32(float(text)))


class ArpaModel:
  """An ARPA n-gram model: ``prob[(w1, .., wn)] = (log10 p, log10 backoff)``, float32-rounded."""

  def __init__(self, text):
    lines = text.splitlines()
    i = 0
    while lines[i].strip() != '\\data\\':
      i += 1
    i += 1
    self.counts = {}
    while lines[i].strip():
      n, c = lines[i].strip()[len('ngram '):].split('=')
      self.counts[int(n)] = int(c)
      i += 1
    self.order = max(self.counts)
    self.prob = {}
    n = 0
    for line in lines[i:]:
      line = line.strip()
      if not line:
        continue
      if line.startswith('\\') and line.endswith('-grams:'):
        n = int(line[1:-len('-grams:')])
        continue
      if line == '\\end\\':
        break
      f = line.split()
      words = tuple(w.lower() for w in f[1:1 + n])
      self.prob[words] = (_f32(f[0]), _f32(f[n + 1]) if len(f) == n + 2 else 0.0)
    for special in ('<unk>', '<s>', '</s>'):
      self.prob.setdefault((special,), (-100.0, 0.0))
    self.vocab = {w[0] for w in self.prob if len(w) == 1 and w[0] and all(ch in LETTERS for ch in w[0])}
    self.min_prefix = {}
    for w in self.vocab:
      p = self.prob[(w,)][0]
      for k in range(1, len(w) + 1):
        self.min_prefix[w[:k]] = min(self.min_prefix.get(w[:k], math.inf), p)

  @classmethod
  def load(cls, path):
    opener = gzip.open if str(path).endswith('.gz') else open
    with opener(path, 'rt', encoding='utf-8') as f:
      return cls(f.read())

  def logp(self, ctx, w):
    """log10 p(w | ctx): p(h w) if listed, else bo(h) + p(w | h[1:]) (a missing backoff counts 0); unknown words are <unk>."""
    w = w if (w,) in self.prob else '<unk>'
    h = tuple(c if (c,) in self.prob else '<unk>' for c in ctx)
    h = h[max(0, len(h) - (self.order - 1)):]
    return self._backoff(h, w)

  def _backoff(self, h, w):
    hit = self.prob.get(h + (w,))
    if hit is not None:
      return hit[0]
    return self.prob.get(h, (0.0, 0.0))[1] + self._backoff(h[1:], w)      # h is not empty: every unigram is listed


class Scorer:
  """The LM state of prefixes (cached by prefix) and the deltas of the spec above."""

  def __init__(self, lm, word_count_weight=0.0, valid_word_count_weight=2.3, oov_score=-1000.0):
    self.lm, self.wcw, self.vwcw, self.oov = lm, word_count_weight, valid_word_count_weight, oov_score
    root_ctx = ('<s>',)[:max(lm.order - 1, 0)]
    self.states = {(): (root_ctx, '', 0.0, 0.0)}       # prefix -> (ctx, incomplete word, lm_score, score)

  def _word(self, ctx, word, lm_score):
    """Scores a completed word: (new ctx, new lm_score)."""
    valid = word in self.lm.vocab
    w = word if valid else '<unk>'
    s = self.lm.logp(ctx, w) + self.wcw + (self.vwcw if valid else 0.0)
    ctx = ctx + (w,)
    ctx = ctx[max(0, len(ctx) - (self.lm.order - 1)):]
    return ctx, lm_score + s

  def state(self, prefix):
    st = self.states.get(prefix)
    if st is None:
      ctx, word, lm_score, _ = self.state(prefix[:-1])
      c = prefix[-1]
      if c == SPACE:
        ctx, lm_score = self._word(ctx, word, lm_score)
        st = (ctx, '', lm_score, lm_score)
      else:
        word = word + LETTERS[c]
        st = (ctx, word, lm_score, lm_score + self.lm.min_prefix.get(word, self.oov))
      self.states[prefix] = st
    return st

  def delta(self, prefix):
    return self.state(prefix)[3] - self.state(prefix[:-1])[3]

  def end_delta(self, prefix):
    ctx, word, lm_score, score = self.state(prefix)
    if word:
      ctx, lm_score = self._word(ctx, word, lm_score)
    return lm_score + self.lm.logp(ctx, '</s>') - score


def _transform(logits_tm, input_transform):
  logits_tm = np.asarray(logits_tm, dtype=np.float64)
  if input_transform == 'log10_softmax':
    z = logits_tm - logits_tm.max(axis=-1, keepdims=True)
    sm = np.exp(z) / np.exp(z).sum(axis=-1, keepdims=True)
    return np.log(sm + 1e-8) / math.log(10)
  if input_transform not in (None, 'logits'):
    raise ValueError(input_transform)
  return logits_tm


def lm_beam_search_decode(logits_tm, seq_lens, lm, beam_width=100, input_transform=None, lm_weight=0.8, word_count_weight=0.0,
                          valid_word_count_weight=2.3, oov_score=-1000.0):
  """The LM-scored prefix beam search (top path) -> (list of id lists, log_prob [B, 1]).  logits_tm [T, B, 29]."""
  logits_tm = _transform(logits_tm, input_transform)
  T, B, C = logits_tm.shape
  assert C == SPACE + 2, 'classes a-z \' space blank'
  blank, ninf = C - 1, -np.inf
  lse = np.logaddexp
  lw = lm_weight
  out, score = [], np.zeros((B, 1))
  for b in range(B):
    sc = Scorer(lm, word_count_weight, valid_word_count_weight, oov_score)
    beams = [((), 0.0, ninf)]
    for t in range(min(int(seq_lens[b]), T)):
      row = logits_tm[t, b]
      lp = row - row.max()
      lp = lp - math.log(np.exp(lp).sum())
      slot_of = {pre: i for i, (pre, _, _) in enumerate(beams)}
      cands = []
      for slot, (pre, pb, pl) in enumerate(beams):
        tot = lse(pb, pl)
        stay_b = tot + lp[blank]
        stay_l = ninf
        if pre:
          mass = pl
          if pre[:-1] in slot_of:
            ppre, ppb, ppl = beams[slot_of[pre[:-1]]]
            mass = lse(mass, (ppb if (ppre and ppre[-1] == pre[-1]) else lse(ppb, ppl)) + lw * sc.delta(pre))
          stay_l = mass + lp[pre[-1]]
        cands.append((lse(stay_b, stay_l), slot * C + blank, pre, stay_b, stay_l))
        for c in range(C - 1):
          child = pre + (c,)
          if child in slot_of:
            continue
          v = lp[c] + ((pb if (pre and pre[-1] == c) else tot) + lw * sc.delta(child))
          cands.append((v, slot * C + c, child, ninf, v))
      cands = [x for x in cands if x[0] > ninf]
      cands.sort(key=lambda x: (-x[0], x[1]))
      beams = [(pre, pb, pl) for _, _, pre, pb, pl in cands[:beam_width]]
    totals = [lse(pb, pl) + lw * sc.end_delta(pre) for pre, pb, pl in beams]
    best = int(np.argmax(totals))                      # first maximum: ties go to the lower rank
    out.append([int(i) for i in beams[best][0]])
    score[b, 0] = totals[best]
  return out, score


def lm_free_equivalent(logits_tm, seq_lens, beam_width, input_transform=None):
  """The recursion this one extends (what it must return with every weight 0)."""
  return O.ctc_beam_search_decode(logits_tm, seq_lens, beam_width, input_transform=input_transform)


def words_to_ids(text):
  return [LETTERS.index(ch) if ch != ' ' else SPACE for ch in text]


def ids_to_text(ids):
  return ''.join(' ' if i == SPACE else LETTERS[i] for i in ids)


def random_arpa(seed, words, counts, backoff_share=0.7, extra_words=()):
  """A random ARPA model (text) from a seed: `words` unigrams spelled in [a-z'] (plus `extra_words`), counts[k] n-grams of order
  k + 2, each extending a listed n-gram of the order below by a random word; backoffs on a share of the lower orders."""
  rng = np.random.default_rng(seed)
  letters = np.array(list(LETTERS[:26]))
  vocab = set()
  while len(vocab) < words:
    n = int(rng.integers(1, 9))
    vocab.add(''.join(rng.choice(letters, n)))
  vocab = sorted(vocab - set(extra_words)) + list(extra_words)
  order = 1 + len(counts)
  lines = ['\\data\\', 'ngram 1={}'.format(len(vocab) + 3)] + ['ngram {}={}'.format(k + 2, c) for k, c in enumerate(counts)] + ['']
  fmt = lambda v: '{:.4f}'.format(v)

  def entry(p, gram, has_bo):
    bo = '\t' + fmt(-rng.uniform(0, 1)) if has_bo and rng.random() < backoff_share else ''
    return fmt(p) + '\t' + ' '.join(gram) + bo

  lines.append('\\1-grams:')
  lines.append(entry(-1.5, ('</s>',), False))
  lines.append(entry(-99, ('<s>',), order > 1))
  lines.append(entry(-4.0, ('<unk>',), order > 1))
  for w in vocab:
    lines.append(entry(-rng.uniform(1, 6), (w,), order > 1))
  grams = [tuple(['<s>'])] + [(w,) for w in vocab]
  ends = vocab + ['</s>']
  for k, c in enumerate(counts):
    n = k + 2
    lines += ['', '\\{}-grams:'.format(n)]
    made = set()
    while len(made) < c:
      g = grams[int(rng.integers(len(grams)))] + (ends[int(rng.integers(len(ends)))],)
      if g[-1] == '</s>' and len(made) % 7:
        continue
      made.add(g)
    made = sorted(made)
    for g in made:
      lines.append(entry(-rng.uniform(0.05, 3), g, n < order))
    grams = [g for g in made if g[-1] != '</s>'] or grams
  lines += ['', '\\end\\', '']
  return '\n'.join(lines)
