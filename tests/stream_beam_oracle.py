"""The CTC prefix beam searches carried across steps: the float64 specification of what a stream reports after n frames.

``tests/nbest_oracle.py::final_sets`` restated so that it yields the beam after EVERY frame (tests/test_stream_beam_cpu.py pins
its end to ``lm_oracle.lm_beam_search_decode`` and ``w2l_oracle.ctc_beam_search_decode``).  From the beam after n frames:

  - the running hypothesis: entry 0 of the set, which is ranked by (total desc, candidate key asc) -- the running total, no
    end-of-utterance terms;
  - the stable length: the length of the longest common prefix, label by label, of all live entries.  Every entry of a later set
    extends an entry of this one, so these labels can never change;
  - at the end of the utterance the whole-utterance result: LM-free entry 0; with a model every entry gains ``lm_weight *`` its
    end-of-utterance delta and the best total wins, ties to the lower rank.

``dtype=np.float32`` runs the recursion's arithmetic in float32 (as in nbest_oracle): the tests use it to vet the inputs on which
the device is asked for equality.
"""
import numpy as np

from tests import lm_oracle as L
from tests import nbest_oracle as NB


def beams_by_frame(logits_tc, length, beam_width, input_transform=None, lm=None, lm_weight=0.8, word_count_weight=0.0,
                   valid_word_count_weight=2.3, oov_score=-1000.0, dtype=np.float64):
  """One utterance, logits [T, C]: yields (n, beams, scorer) for n = 0 .. min(length, T), beams = [(prefix, p_blank, p_label)]
  in the set's order after n frames."""
  logits_tc = np.asarray(logits_tc)
  T, C = logits_tc.shape
  if lm is not None:
    assert C == L.SPACE + 2, 'classes a-z \' space blank'
  lp_all = NB._rows(logits_tc[:, None, :], input_transform, dtype)[:, 0]
  f = dtype
  blank, ninf = C - 1, f(-np.inf)
  lse = lambda a, b: f(np.logaddexp(f(a), f(b)))
  lw = f(lm_weight)
  sc = L.Scorer(lm, word_count_weight, valid_word_count_weight, oov_score) if lm is not None else None
  beams = [((), f(0.0), ninf)]
  yield 0, beams, sc
  for t in range(min(int(length), T)):
    lp = lp_all[t]
    slot_of = {e[0]: i for i, e in enumerate(beams)}
    cands = []
    for slot, (pre, pb, pl) in enumerate(beams):
      tot = lse(pb, pl)
      stay_b = f(tot + lp[blank])
      stay_l = ninf
      if pre:
        mass = pl
        if pre[:-1] in slot_of:
          ppre, ppb, ppl = beams[slot_of[pre[:-1]]]
          inflow = ppb if (bool(ppre) and ppre[-1] == pre[-1]) else lse(ppb, ppl)
          mass = lse(mass, f(inflow + lw * f(sc.delta(pre))) if sc is not None else inflow)
        stay_l = f(mass + lp[pre[-1]])
      cands.append((lse(stay_b, stay_l), slot * C + blank, pre, stay_b, stay_l))
      for c in range(C - 1):
        child = pre + (c,)
        if child in slot_of:
          continue
        base = pb if (bool(pre) and pre[-1] == c) else tot
        v = f(lp[c] + f(base + lw * f(sc.delta(child)))) if sc is not None else f(base + lp[c])
        cands.append((v, slot * C + c, child, ninf, v))
    cands = [x for x in cands if x[0] > ninf]
    cands.sort(key=lambda x: (-x[0], x[1]))
    beams = [x[2:] for x in cands[:beam_width]]
    yield t + 1, beams, sc


def running_best(beams):
  return list(beams[0][0])


def stable_length(beams):
  """Length of the label-wise longest common prefix of the set's prefixes."""
  first = beams[0][0]
  n = min(len(e[0]) for e in beams)
  for pre, _, _ in beams[1:]:
    k = 0
    while k < n and pre[k] == first[k]:
      k += 1
    n = k
  return n


def final_result(beams, sc, lm_weight=0.8, dtype=np.float64):
  """(ids, log_prob) of the whole-utterance search from its last set."""
  f = dtype
  totals = [f(np.logaddexp(f(pb), f(pl))) for _, pb, pl in beams]
  if sc is not None:
    totals = [f(t + f(lm_weight) * f(sc.end_delta(pre))) for t, (pre, _, _) in zip(totals, beams)]
    best = int(np.argmax(totals))                       # first maximum: ties go to the lower rank
  else:
    best = 0
  return [int(i) for i in beams[best][0]], float(totals[best])


def trace(logits_tc, length, beam_width, dtype=np.float64, **kw):
  """What a stream reports: ``hyp[n]`` / ``stable[n]`` after n frames (n = 0 .. length), ``members[n]`` the set's prefixes, and
  ``final`` = (ids, log_prob) of the whole utterance."""
  hyp, stable, members = [], [], []
  for n, beams, sc in beams_by_frame(logits_tc, length, beam_width, dtype=dtype, **kw):
    hyp.append(running_best(beams))
    stable.append(stable_length(beams))
    members.append(frozenset(e[0] for e in beams))
  return dict(hyp=hyp, stable=stable, members=members, final=final_result(beams, sc, kw.get('lm_weight', 0.8), dtype))
