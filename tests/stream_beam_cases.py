"""Inputs shared by tests/test_stream_beam_cpu.py and tests/test_gpu_stream_beam.py: the utterances of
``test_gpu_lm_beam.py::_cases`` (T = 80, five utterances with the lengths 0 and 1 among them, C = 29), a C = 5 case for the LM-free
search, and the configurations on which the GPU test compares partial results EXACTLY with the float64 specification -- the CPU
test shows that on these the specification's beams do not hinge on the precision of the search."""
import os

import numpy as np

from tests import lm_oracle as L
from tests import stream_beam_oracle as SB
from tests.test_gpu_lm_beam import SENTENCE_WORDS, TINY, _cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cases29(seed):
  return _cases(seed)


def cases5(seed):
  """LM-free, five classes: the same shape of batch (a peaky utterance, a blank-heavy one, lengths 0 and 1)."""
  rng = np.random.default_rng(seed)
  T, B, C = 80, 5, 5
  logits = rng.standard_normal((T, B, C)) * 2.0
  logits[:, 2, C - 1] += 3.0
  return logits.astype(np.float32), [80, 41, 77, 0, 1]


_ARPA = {}


def arpa_text(order):
  """order 3: the hand-written model; others: the seeded random model of test_gpu_lm_beam.py::_model."""
  if order not in _ARPA:
    if order == 3:
      with open(TINY) as f:
        _ARPA[order] = f.read()
    else:
      _ARPA[order] = L.random_arpa(100 + order, 150, [400, 300, 200, 100][:order - 1], extra_words=SENTENCE_WORDS)
  return _ARPA[order]


# (name, beam, LM order or 0, input transform, classes, seed): the partials of these are compared exactly
EXACT = [
    ('free16', 16, 0, None, 29, 3),
    ('free5c', 16, 0, 'log10_softmax', 5, 4),
    ('lm16', 16, 3, 'log10_softmax', 29, 5),
    ('lm100', 100, 3, None, 29, 6),
]


def exact_inputs(name):
  _, beam, order, transform, C, seed = next(c for c in EXACT if c[0] == name)
  logits, lens = cases29(seed) if C == 29 else cases5(seed)
  return logits, lens, beam, order, transform


_TRACES = {}


def traces(name, dtype=np.float64):
  """The specification's trace of every utterance of an EXACT configuration (computed once per process)."""
  key = (name, np.dtype(dtype).name)
  if key not in _TRACES:
    logits, lens, beam, order, transform = exact_inputs(name)
    lm = L.ArpaModel(arpa_text(order)) if order else None
    _TRACES[key] = [SB.trace(logits[:, b].astype(np.float64), lens[b], beam, dtype=dtype, input_transform=transform, lm=lm)
                    for b in range(logits.shape[1])]
  return _TRACES[key]
