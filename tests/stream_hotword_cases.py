"""Inputs shared by tests/test_stream_hotwords_cpu.py and tests/test_gpu_stream_hotwords.py: three streams of unequal lengths whose
logits spell, with noise, text in which the phrase sets' phrases open, fail and complete; the phrase sets (overlapping phrases, a
phrase that is a prefix of another, a set with another weight); and the configurations on which the GPU test compares partial
results with the float64 specification (tests/stream_hotword_oracle.py) -- the CPU test shows that on these no selection hinges on
less than the comparison's tolerance."""
import numpy as np

from tests import lm_oracle as L
from tests import stream_hotword_oracle as SH
from tests.test_lm_oracle_cpu import word_logits

T, POOL = 60, 80
LENS = [52, 30, 41]                                     # output frames of the three streams
STREAM_SETS = [1, 2, 1]                                 # the phrase set (index into HotwordSets) of each stream
TAU = 1e-4                                              # the margin of tests/test_hotwords_cpu.py (nbest_oracle.TAU)

# 29 classes: a-z ' space blank.  Set 1: 'cat' is a prefix of 'cat s'; 'at s' overlaps both.  Set 2 has another weight.  (The weights are small enough that the
# hypotheses still follow the audio: 'the cat' then breaks off the match of 'the ma'.)
TEXTS29 = ['the cat sat on the mat', 'on the mat', 'a cat on the mat']
SETS29 = [(['cat', 'cat s', 'at s', 'the ma', 'on', 'zeb'], 0.4), (['the', 'he m', 'mat', 'n t', 'dog'], 0.25)]
# 5 classes: labels 0..3 and the blank.  The texts are label strings; set 1 nests (0, 1) in (0, 1, 2) and overlaps it with (1, 2, 3); the
# third text opens (2, 0, 3, 3, 0, 1) and breaks it off.
TEXTS5 = [(0, 1, 2, 3, 0, 1, 3, 2, 2, 1, 0, 1, 2, 0, 3, 3, 0, 1), (2, 3, 0, 1, 2, 2, 3, 1, 0, 1), (3, 0, 1, 1, 2, 0, 3, 1, 0, 1, 2, 3, 1, 2)]
SETS5 = [([(0, 1), (0, 1, 2), (1, 2, 3), (3, 2, 2), (2, 0, 3, 3, 0, 1)], 0.25), ([(1, 0), (2, 3), (3, 0, 1, 1), (0, 0)], 0.15)]


def phrase_sets(C):
  """[(phrases as id tuples, weight)] of the real sets 1, 2 (set 0 is the empty one)."""
  if C == 29:
    return [([tuple(L.words_to_ids(p)) for p in phrases], w) for phrases, w in SETS29]
  return [([tuple(p) for p in phrases], w) for phrases, w in SETS5]


def streams(C, seed, noise=1.0, peak=3.0):
  """-> (logits float32 [T, 3, C], LENS): stream s spells its text (three frames per label: two of the label, one blank) under
  noise; rows past the text are noise."""
  rng = np.random.default_rng(seed)
  logits = rng.standard_normal((T, 3, C)) * 2.0
  for s in range(3):
    if C == 29:
      w = word_logits(TEXTS29[s], rng, frames_per_char=2, gap=1, noise=noise, peak=peak)
    else:
      rows = []
      for c in TEXTS5[s]:
        for k in (c, c, C - 1):
          r = rng.standard_normal(C) * noise
          r[k] += peak
          rows.append(r)
      w = np.array(rows)
    n = min(len(w), T)
    logits[:n, s] = w[:n]
  return logits.astype(np.float32), list(LENS)


def what_happened(phrases, ids):
  """-> (opened, failed, completed) along the label string ``ids`` under a phrase set: a partial match was open, credit was given
  back, a phrase was banked -- by the specification's scan (hotword_oracle.Scan)."""
  from tests import hotword_oracle as H
  during, _ = H.Scan(phrases).scan(tuple(ids))
  opened = any(r > 0 for _, r in during)
  credit = [0] + [m + r for m, r in during]
  failed = any(b < a for a, b in zip(credit, credit[1:]))
  completed = bool(during) and during[-1][0] > 0
  return opened, failed, completed


# (name, beam, with the trigram model, input transform, classes, seed): the partials of these are compared with the specification.
# The seeds were picked on the specification alone, for the two conditions test_stream_hotwords_cpu.py tests.
EXACT = [
    ('free16', 16, False, None, 29, 2),
    ('free5c', 16, False, 'log10_softmax', 5, 3),
    ('lm16', 16, True, 'log10_softmax', 29, 1),
    ('lm100', 100, True, None, 29, 1),
]


def exact_inputs(name):
  _, beam, with_lm, transform, C, seed = next(c for c in EXACT if c[0] == name)
  logits, lens = streams(C, seed)
  return logits, lens, beam, with_lm, transform


_TRACES = {}


def traces(name, dtype=np.float64):
  """The specification's trace of every stream of an EXACT configuration, each under its own phrase set (once per process)."""
  key = (name, np.dtype(dtype).name)
  if key not in _TRACES:
    from tests.test_nbest_cpu import TINY
    logits, lens, beam, with_lm, transform = exact_inputs(name)
    lm = L.ArpaModel.load(TINY) if with_lm else None
    sets = [((), 1.0)] + phrase_sets(logits.shape[2])
    _TRACES[key] = [SH.trace(logits[:, s].astype(np.float64), lens[s], beam, dtype=dtype, input_transform=transform, lm=lm,
                             phrases=sets[STREAM_SETS[s]][0], weight=sets[STREAM_SETS[s]][1]) for s in range(len(lens))]
  return _TRACES[key]
