"""Hotword biasing of the CTC prefix beam searches carried across steps: the float64 specification of what a biased stream reports.

``tests/stream_beam_oracle.py`` with the second scorer of ``tests/hotword_oracle.py`` (`Bias`): the gain of a prefix's last label goes
wherever the LM's delta goes -- child candidates and the stay candidate's parent inflow, after the LM's term -- and at the end of the
utterance every entry adds ``Bias.end_delta`` after the LM's end-of-utterance delta, with or without a model; the best total then
wins, ties to the lower rank (``hotword_oracle.final_sets``, whose first entry `final` restates).

The search is an object that is fed rows (`Search.feed`), so that the specification itself can be cut: what it reports after n frames
does not depend on how the n frames arrived.

  - running hypothesis: entry 0 of the set with its running total, which carries the credit lent to an open match;
  - stable length: the label-wise longest common prefix of all live entries;
  - `margins`: per frame the smallest gap between two candidates that DECIDE something a stream reports -- the best against the
    second (the hypothesis), the last kept against the first dropped (the set, hence the stable length) -- and `final_margin`, the
    best final total against the second.  The GPU comparison uses inputs whose margins all exceed its tolerance.

``dtype=np.float32`` runs the recursion in float32, as in stream_beam_oracle.
"""
import numpy as np

from tests import hotword_oracle as H
from tests import lm_oracle as L
from tests import nbest_oracle as NB
from tests import stream_beam_oracle as SB


class Search:
  """One stream.  ``phrases`` / ``weight``: the stream's own phrase set (none: the unbiased search of stream_beam_oracle)."""

  def __init__(self, num_classes, beam_width, phrases=(), weight=1.0, input_transform=None, lm=None, lm_weight=0.8,
               word_count_weight=0.0, valid_word_count_weight=2.3, oov_score=-1000.0, dtype=np.float64):
    if lm is not None:
      assert num_classes == L.SPACE + 2, 'classes a-z \' space blank'
    self.C, self.W, self.transform, self.f = num_classes, beam_width, input_transform, dtype
    self.sc = L.Scorer(lm, word_count_weight, valid_word_count_weight, oov_score) if lm is not None else None
    self.lw = dtype(lm_weight)
    self.hot = H.Bias(phrases, weight)
    self.beams = [((), dtype(0.0), dtype(-np.inf))]
    self.frames, self.margins = 0, []

  def _entered(self, base, prefix):
    f = self.f
    if self.sc is not None:
      base = f(base + self.lw * f(self.sc.delta(prefix)))
    return f(base + f(self.hot.delta(prefix)))

  def feed(self, logits_tc):
    """Decode the rows [t, C] (any number, 0 included) on top of what was fed before."""
    logits_tc = np.asarray(logits_tc)
    if not len(logits_tc):
      return
    f, C = self.f, self.C
    blank, ninf = C - 1, f(-np.inf)
    lse = lambda a, b: f(np.logaddexp(f(a), f(b)))
    for lp in NB._rows(logits_tc[:, None, :], self.transform, f)[:, 0]:
      beams = self.beams
      slot_of = {e[0]: i for i, e in enumerate(beams)}
      cands = []
      for slot, (pre, pb, pl) in enumerate(beams):
        tot = lse(pb, pl)
        stay_b, stay_l = f(tot + lp[blank]), ninf
        if pre:
          mass = pl
          if pre[:-1] in slot_of:
            ppre, ppb, ppl = beams[slot_of[pre[:-1]]]
            mass = lse(mass, self._entered(ppb if (bool(ppre) and ppre[-1] == pre[-1]) else lse(ppb, ppl), pre))
          stay_l = f(mass + lp[pre[-1]])
        cands.append((lse(stay_b, stay_l), slot * C + blank, pre, stay_b, stay_l))
        for c in range(C - 1):
          child = pre + (c,)
          if child in slot_of:
            continue
          v = f(lp[c] + self._entered(pb if (bool(pre) and pre[-1] == c) else tot, child))
          cands.append((v, slot * C + c, child, ninf, v))
      cands = [x for x in cands if x[0] > ninf]
      cands.sort(key=lambda x: (-x[0], x[1]))
      gaps = [float(cands[0][0] - cands[1][0])] if len(cands) > 1 else []
      if len(cands) > self.W:
        gaps.append(float(cands[self.W - 1][0] - cands[self.W][0]))
      self.margins.append(min(gaps) if gaps else np.inf)
      self.beams = [x[2:] for x in cands[:self.W]]
      self.frames += 1

  def report(self):
    """(hypothesis, stable length, running log-probability) of the open stream."""
    pre, pb, pl = self.beams[0]
    return [int(i) for i in pre], SB.stable_length(self.beams), float(np.logaddexp(self.f(pb), self.f(pl)))

  def members(self):
    return frozenset(e[0] for e in self.beams)

  def final(self):
    """(ids, log_prob, margin) of the whole-utterance biased search from the live set."""
    f = self.f
    totals = []
    for pre, pb, pl in self.beams:
      t = f(np.logaddexp(f(pb), f(pl)))
      if self.sc is not None:
        t = f(t + self.lw * f(self.sc.end_delta(pre)))
      totals.append(f(t + f(self.hot.end_delta(pre))))
    best = int(np.argmax(totals))                         # first maximum: ties go to the lower rank
    rest = [float(totals[best] - t) for i, t in enumerate(totals) if i != best]
    return [int(i) for i in self.beams[best][0]], float(totals[best]), (min(rest) if rest else np.inf)


def trace(logits_tc, length, beam_width, **kw):
  """What a stream reports, frame by frame: ``hyp[n]`` / ``stable[n]`` / ``logp[n]`` after n frames (n = 0 .. length),
  ``members[n]``, ``margins[n - 1]`` of frame n, and ``final`` = (ids, log_prob), ``final_margin`` of the whole utterance."""
  logits_tc = np.asarray(logits_tc)
  s = Search(logits_tc.shape[1], beam_width, **kw)
  out = dict(hyp=[], stable=[], logp=[], members=[])

  def note():
    h, st, lp = s.report()
    out['hyp'].append(h)
    out['stable'].append(st)
    out['logp'].append(lp)
    out['members'].append(s.members())

  note()
  for t in range(min(int(length), len(logits_tc))):
    s.feed(logits_tc[t:t + 1])
    note()
  ids, logp, margin = s.final()
  out.update(final=(ids, logp), final_margin=margin, margins=list(s.margins))
  return out
