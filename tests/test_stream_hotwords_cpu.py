"""Hotword biasing of the streaming beam searches without a GPU: the concatenated tables of `hotwords.HotwordSets` against the
specification (tests/hotword_oracle.py), the streaming specification's own properties (tests/stream_hotword_oracle.py), the margins
of the cases the GPU comparison uses (tests/stream_hotword_cases.py), and the exports and the CLI surface."""
import importlib.machinery
import importlib.util
import os

import numpy as np
import pytest

from tests import hotword_oracle as H
from tests import lm_oracle as L
from tests import stream_beam_oracle as SB
from tests import stream_hotword_cases as HC
from tests import stream_hotword_oracle as SH
from tests.test_nbest_cpu import ROOT, TINY


# ---- the set tables ----------------------------------------------------------------------------------------------------------------

SET_LISTS = [
    [(['cat', 'cat s', 'at s'], 1.0), (['the', 'he m', 'mat'], 0.6)],                                  # a prefix pair, overlaps, another weight
    [([(0, 1), (0, 1, 2), (1, 2, 3)], 1.0), ([(1, 0), (2, 3), (0, 0)], 0.5), ([(2,), (2, 2, 2, 1)], 2.5)],
    [HC.SETS29[0], HC.SETS29[1]], [HC.SETS5[0], HC.SETS5[1]],
]


@pytest.mark.parametrize('sets', SET_LISTS)
def test_set_tables_are_the_oracle_tables_shifted(sets):
  from speecht_amd.hotwords import Hotwords, HotwordSets
  hs = HotwordSets([Hotwords(list(p), w) for p, w in sets])
  assert len(hs) == len(sets) + 1 and hs.base[0] == 0 and hs.base[1] == 1 and hs.n_states == hs.base[-1] == len(hs.next)
  assert hs.next.dtype == np.int32 and hs.gain.dtype == np.float32 and hs.fin.dtype == np.float32
  assert hs.next.shape == hs.gain.shape == (hs.n_states, 32) and hs.fin.shape == (hs.n_states,)
  # set 0: one state, nowhere to go, nothing to earn
  assert (hs.next[0] == 0).all() and not hs.gain[0].any() and hs.fin[0] == 0
  rng = np.random.default_rng(5)
  for k, (phrases, w) in enumerate(sets, 1):
    nxt, gain, fin = H.tables(phrases, w)
    lo, hi = int(hs.base[k]), int(hs.base[k + 1])
    assert hi - lo == len(nxt) and hs.root(k) == lo
    assert np.array_equal(hs.next[lo:hi], nxt + lo) and hs.gain[lo:hi].tobytes() == gain.tobytes() and hs.fin[lo:hi].tobytes() == fin.tobytes()
    assert hs.tables(k).phrases == [tuple(L.words_to_ids(p)) if isinstance(p, str) else tuple(p) for p in phrases]
    # a scan from the set's root never leaves the set's rows and scores what the rules on strings score
    letters = sorted({c for p in H.as_phrases(phrases) for c in p})
    for _ in range(40):
      x = [letters[i] for i in rng.integers(0, len(letters), int(rng.integers(0, 20)))]
      n, s, during = lo, 0.0, []
      for c in x:
        s += float(hs.gain[n, c])
        n = int(hs.next[n, c])
        assert lo <= n < hi
        during.append(s)
      want_during, want_final = H.scores(phrases, w, x)
      assert during == pytest.approx(want_during, abs=1e-5) and s + float(hs.fin[n]) == pytest.approx(want_final, abs=1e-5)
      assert (during, s + float(hs.fin[n])) == H.table_scan((nxt, gain, fin), x)


def test_sets_validate():
  from speecht_amd import hotwords as hw
  with pytest.raises(hw.HotwordError, match='list of Hotwords'):
    hw.HotwordSets(hw.Hotwords(['cat']))
  hs = hw.HotwordSets([['cat'], hw.Hotwords(['dog'], 2.0)])              # a plain phrase list becomes a Hotwords of weight 1
  assert len(hs) == 3 and hs.sets[1].weight == 1.0 and hs.sets[2].weight == 2.0 and hs.n_states == 1 + 4 + 4
  for bad in (-1, 3, 1.0, None):
    with pytest.raises(hw.HotwordError, match='sets 0..2'):
      hs.root(bad)
  assert len(hw.HotwordSets([])) == 1 and hw.HotwordSets([]).n_states == 1


def test_sets_share_the_limit_on_states(monkeypatch):
  """MAX_STATES bounds the concatenation, not each set: two sets that fit alone are refused together."""
  from speecht_amd import hotwords as hw
  monkeypatch.setattr(hw, 'MAX_STATES', 8)
  one, two = hw.Hotwords(['cat']), hw.Hotwords(['dog', 'do'])      # 4 states each
  assert hw.HotwordSets([one]).n_states == 5 and hw.HotwordSets([one, [[1, 2]]]).n_states == 8
  with pytest.raises(hw.HotwordError, match='9 trie nodes in all, at most 8'):
    hw.HotwordSets([one, two])


def test_stream_beam_takes_hotwords():
  from speecht_amd import hotwords as hw
  from speecht_amd.streaming import StreamBeam, StreamError
  one = StreamBeam(hotwords=hw.Hotwords(['cat']))
  assert isinstance(one.hotwords, hw.HotwordSets) and len(one.hotwords) == 2 and one.default_set == 1 and one.beam_width == 16
  many = StreamBeam(hotwords=hw.HotwordSets([['cat'], ['dog']]))
  assert len(many.hotwords) == 3 and many.default_set == 0
  assert StreamBeam().hotwords is None
  with pytest.raises(StreamError, match='Hotwords'):
    StreamBeam(hotwords=['cat'])


# ---- the streaming specification ------------------------------------------------------------------------------------------------------

def test_without_phrases_the_specification_is_the_unbiased_one():
  logits, lens = HC.streams(5, 3)
  for s in range(3):
    want = SB.trace(logits[:, s].astype(np.float64), lens[s], 8, input_transform='log10_softmax')
    for phrases, w in (((), 1.0), (HC.phrase_sets(5)[0][0], 0.0)):
      got = SH.trace(logits[:, s].astype(np.float64), lens[s], 8, input_transform='log10_softmax', phrases=phrases, weight=w)
      assert got['hyp'] == want['hyp'] and got['stable'] == want['stable'] and got['members'] == want['members']
      assert got['final'] == want['final']


@pytest.mark.parametrize('with_lm', [False, True])
def test_the_specification_ends_in_the_whole_utterance_oracle(with_lm):
  """Its final is the first entry of hotword_oracle.final_sets, total included."""
  lm = L.ArpaModel.load(TINY) if with_lm else None
  logits, lens = HC.streams(29, 2)
  for k, (phrases, w) in enumerate(HC.phrase_sets(29)):
    sets = H.final_sets(logits.astype(np.float64), lens, 8, lm=lm, hotwords=phrases, hotword_weight=w)
    for s in range(3):
      tr = SH.trace(logits[:, s].astype(np.float64), lens[s], 8, lm=lm, phrases=phrases, weight=w)
      assert tuple(tr['final'][0]) == sets[s][0][0] and tr['final'][1] == sets[s][0][1]


@pytest.mark.parametrize('C,with_lm', [(5, False), (29, False), (29, True)])
def test_cutting_the_frames_changes_nothing(C, with_lm):
  lm = L.ArpaModel.load(TINY) if with_lm else None
  logits, lens = HC.streams(C, 7)
  rng = np.random.default_rng(C)
  for s in range(3):
    phrases, w = HC.phrase_sets(C)[s % 2]
    kw = dict(phrases=phrases, weight=w, lm=lm, input_transform='log10_softmax' if with_lm else None)
    whole = SH.trace(logits[:, s].astype(np.float64), lens[s], 8, **kw)
    assert all(a <= b for a, b in zip(whole['stable'], whole['stable'][1:]))            # stable lengths never shrink
    assert all(st <= len(h) for st, h in zip(whole['stable'], whole['hyp']))
    for pattern in ([1], [lens[s]], rng.integers(1, 9, 40).tolist()):
      search, at, k = SH.Search(C, 8, **kw), 0, 0
      while at < lens[s]:
        n = min(pattern[k % len(pattern)], lens[s] - at)
        search.feed(logits[at:at + n, s].astype(np.float64))
        at, k = at + n, k + 1
        hyp, stable, logp = search.report()
        assert hyp == whole['hyp'][at] and stable == whole['stable'][at] and logp == whole['logp'][at], (s, at)
        assert search.members() == whole['members'][at]
      assert search.final()[:2] == whole['final']
    # credit is carried while the stream is open: where both searches report the same text and that text has earned some (banked
    # or lent), the biased running total exceeds the unbiased one's by about it (the two beams prune differently: half is asked)
    plain = SH.trace(logits[:, s].astype(np.float64), lens[s], 8, **dict(kw, phrases=()))
    lent = [(whole['logp'][n] - plain['logp'][n], H.scores(phrases, w, whole['hyp'][n])[0][-1]) for n in range(1, lens[s] + 1)
            if whole['hyp'][n] and whole['hyp'][n] == plain['hyp'][n]]
    assert any(credit > 0 and more > 0.5 * credit for more, credit in lent), (s, lent)


# ---- the cases of the GPU comparison and their margins ---------------------------------------------------------------------------------

def test_the_cases_have_the_asked_shapes():
  assert len(HC.LENS) == 3 and len(set(HC.LENS)) == 3 and all(30 <= n <= 60 for n in HC.LENS) and HC.POOL == 80
  for C in (29, 5):
    sets = HC.phrase_sets(C)
    assert len(sets) == 2 and sets[0][1] != sets[1][1]
    for phrases, _ in sets:
      assert 3 <= len(phrases) <= 8 and all(2 <= len(p) <= 6 for p in phrases)
    first = sets[0][0]
    assert any(a != b and b[:len(a)] == a for a in first for b in first)                # a phrase that is a prefix of another
    assert any(a[-k:] == b[:k] for a in first for b in first if a != b for k in (1, 2, 3) if len(a) > k and len(b) > k)   # overlap
  assert {c[1] for c in HC.EXACT} >= {16, 100} and {c[4] for c in HC.EXACT} == {5, 29} and {c[2] for c in HC.EXACT} == {False, True}


@pytest.mark.parametrize('name', [c[0] for c in HC.EXACT])
def test_the_cases_do_not_hinge_on_the_precision(name):
  """float32 and float64 report the same hypotheses and stable lengths, and no two candidates that decide a selection -- the best
  against the second, the last kept against the first dropped, the best final total against the second -- are closer than 1e-4."""
  t64, t32 = HC.traces(name), HC.traces(name, np.float32)
  C = HC.exact_inputs(name)[0].shape[2]
  sets = [((), 1.0)] + HC.phrase_sets(C)
  seen = [False, False, False]
  for s, (a, b) in enumerate(zip(t64, t32)):
    assert a['hyp'] == b['hyp'] and a['stable'] == b['stable'] and a['final'][0] == b['final'][0], (name, s)
    assert a['members'] == b['members']
    margins = a['margins'] + b['margins'] + [a['final_margin'], b['final_margin']]
    assert min(margins) >= HC.TAU, (name, s, min(margins), int(np.argmin(margins)))
    np.testing.assert_allclose(b['logp'], a['logp'], rtol=1e-4, atol=1e-4)
    phrases = sets[HC.STREAM_SETS[s]][0]
    for hyp in a['hyp']:
      seen = [x or y for x, y in zip(seen, HC.what_happened(phrases, hyp))]
  assert seen == [True, True, True], (name, seen)                 # matches open, fail and complete in the hypotheses themselves


# ---- exports and the command line --------------------------------------------------------------------------------------------------

def test_exports_and_header():
  from speecht_amd import _lib
  with open(os.path.join(ROOT, 'include', 'speecht_hip.h')) as f:
    header = f.read()
  for name in ('st_ctc_beam_stream_bias_state_bytes', 'st_ctc_beam_stream_step_bias', 'st_ctc_beam_stream_read_bias',
               'st_ctc_beam_stream_step_pieces_bias'):
    assert name in _lib._SIGNATURES and name + '(' in header, name
  for name in ('step', 'read', 'step_pieces'):                     # the existing signature, then the tables and the roots
    plain, biased = _lib._SIGNATURES['st_ctc_beam_stream_' + name], _lib._SIGNATURES['st_ctc_beam_stream_{}_bias'.format(name)]
    assert biased[0] == plain[0] and biased[1][:-2] == plain[1] and len(biased[1]) == len(plain[1]) + 2
  assert 'roots[s]' in header and 'bias bit' in header


def _cli():
  loader = importlib.machinery.SourceFileLoader('speecht_cli_stream_hotwords', os.path.join(ROOT, 'speecht-cli'))
  spec = importlib.util.spec_from_loader('speecht_cli_stream_hotwords', loader)
  cli = importlib.util.module_from_spec(spec)
  loader.exec_module(cli)
  return cli


def test_cli_stream_parses_the_hotword_flags(tmp_path, capsys):
  from speecht_amd import hotwords as hw
  cli = _cli()
  words = tmp_path / 'words.txt'
  words.write_text('# contacts\nnew york\nZebra\n')
  _, flags = cli.parse(['stream', '--hotwords', str(words), '--hotword', 'the Cat', '--hotword', 'mat', '--hotword-weight', '0.5', 'a.flac'])
  assert flags.hotwords == str(words) and flags.hotword == ['the Cat', 'mat'] and flags.hotword_weight == 0.5
  built = hw.from_flags(flags)
  assert built.weight == 0.5 and built.phrases == [tuple(L.words_to_ids(p)) for p in ('new york', 'zebra', 'the cat', 'mat')]
  _, plain = cli.parse(['stream', 'a.flac'])
  assert hw.from_flags(plain) is None and not hasattr(plain, 'hotword')
  for argv, text in ((['stream', '--hotword-weight', '2', 'a.flac'], 'applies with --hotwords or --hotword only'),
                     (['stream', '--hotword', 'café', 'a.flac'], 'outside the vocabulary'),
                     (['stream', '--hotwords', str(tmp_path / 'none.txt'), 'a.flac'], 'cannot read --hotwords')):
    with pytest.raises(SystemExit):
      cli.main(argv)
    assert text in capsys.readouterr().err
