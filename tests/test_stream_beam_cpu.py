"""The specification of the streamed beam searches (tests/stream_beam_oracle.py): its end is the whole-utterance search of the
two existing oracles, its stable prefix only grows and stays a prefix of everything reported later, and on the inputs the GPU
test compares exactly its beams do not depend on the precision of the arithmetic.  Plus the command line's new flags."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import w2l_oracle as O
from tests import lm_oracle as L
from tests import stream_beam_cases as SC
from tests import stream_beam_oracle as SB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('beam,order,transform', [(1, 3, None), (16, 1, 'log10_softmax'), (16, 3, None), (16, 5, 'log10_softmax'),
                                                  (64, 3, 'log10_softmax')])
def test_the_end_is_the_lm_search(beam, order, transform):
  logits, lens = SC.cases29(10 * beam + order)
  lm = L.ArpaModel(SC.arpa_text(order))
  ref_ids, ref_lp = L.lm_beam_search_decode(logits.astype(np.float64), lens, lm, beam, transform)
  for b in range(len(lens)):
    ids, lp = SB.trace(logits[:, b].astype(np.float64), lens[b], beam, input_transform=transform, lm=lm)['final']
    assert ids == ref_ids[b]
    assert lp == pytest.approx(float(ref_lp[b, 0]), rel=1e-12, abs=1e-12)


@pytest.mark.parametrize('beam,transform,classes', [(1, None, 29), (16, 'log10_softmax', 29), (16, None, 5), (64, None, 29)])
def test_the_end_is_the_lm_free_search(beam, transform, classes):
  logits, lens = SC.cases29(beam) if classes == 29 else SC.cases5(beam)
  ref_ids, ref_lp = O.ctc_beam_search_decode(logits.astype(np.float64), lens, beam, input_transform=transform)
  for b in range(len(lens)):
    ids, lp = SB.trace(logits[:, b].astype(np.float64), lens[b], beam, input_transform=transform)['final']
    assert ids == ref_ids[b]
    assert lp == pytest.approx(float(np.asarray(ref_lp).reshape(len(lens), -1)[b, 0]), rel=1e-12, abs=1e-12)


@pytest.mark.parametrize('name', [c[0] for c in SC.EXACT])
def test_stable_prefix_only_grows_and_is_final(name):
  for tr in SC.traces(name):
    hyp, stable = tr['hyp'], tr['stable']
    assert stable[0] == 0 and hyp[0] == []
    assert all(a <= b for a, b in zip(stable, stable[1:]))
    for n in range(len(hyp)):
      committed = hyp[n][:stable[n]]
      assert len(committed) == stable[n]
      for later in hyp[n:] + [tr['final'][0]]:
        assert later[:stable[n]] == committed, (name, n)
  assert any(max(tr['stable']) > 0 for tr in SC.traces(name))       # (the property is not vacuous on these inputs)


@pytest.mark.parametrize('name', [c[0] for c in SC.EXACT])
def test_exact_inputs_do_not_hinge_on_precision(name):
  """What lets the GPU test ask for equality: in float32 and in float64 the beam has the same members after every frame (and so
  the same common prefix), the same best entry and the same final ids."""
  for b, (a, c) in enumerate(zip(SC.traces(name, np.float64), SC.traces(name, np.float32))):
    assert len(a['members']) == len(c['members'])
    for n, (ma, mc) in enumerate(zip(a['members'], c['members'])):
      assert ma == mc, (name, b, n)
    assert a['hyp'] == c['hyp'] and a['stable'] == c['stable'] and a['final'][0] == c['final'][0], (name, b)


def test_cli_stream_help_names_the_language_model_flags():
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'speecht-cli'), 'stream', '--help'], capture_output=True, text=True, timeout=120)
  assert r.returncode == 0, r.stderr
  for flag in ('--language-model', '--beam-width', '--beam-input', '--lm-weight', '--word-count-weight', '--valid-word-count-weight'):
    assert flag in r.stdout, flag
