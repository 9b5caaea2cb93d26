"""CTC word confidences without a GPU: the float64 specification (tests/conf_oracle.py) against brute-force enumeration of all
frame paths, its properties, the host form st_ctc_word_conf_host against it through every states-per-lane dispatch, the edge
cases, and the host-side word splitter and output formats.

The gate of the host form (and, bit for bit, of the kernel: tests/test_gpu_confidence.py) is 1e-9 ABSOLUTE on log_prob and on
every log_conf.  Reasoning: all terms of the recursion are positive; each of T <= 1 501 frames costs about three roundings of
2^-53 and those of its emission, about 1e-12 on ln P; the oracle's own log-sum-exp at magnitudes up to 1e3 is of that order or
somewhat worse; 1e-9 leaves three decades above both."""
import ctypes
import functools
import io
import json

import numpy as np
import pytest

from tests import align_oracle as AO
from tests import conf_oracle as CO

GATE = 1e-9
C, SPACE = 29, 27

# (largest label, frames) per dispatch of the lattice, as tests/test_gpu_align.py
DISPATCH = [(31, 70), (63, 140), (95, 300), (127, 501), (159, 501), (191, 640), (255, 800), (319, 1000), (383, 1200), (511, 1501)]


def _p(a):
  return ctypes.c_void_p(a.ctypes.data)


def host_conf(logits, labels, seq_lens, space_id=SPACE, max_label_len=None, spans=None):
  """st_ctc_word_conf_host on a dense [B, T, C] batch -> (log_prob [B], log_conf [n_words], status [B], spans [n_words, 3])."""
  from speecht_amd import _lib
  lib = _lib.load()
  logits = np.ascontiguousarray(logits, dtype=np.float32)
  B, T, Cc = logits.shape
  ids, offs = CO.csr(labels)
  spans = CO.batch_spans(labels, space_id) if spans is None else np.ascontiguousarray(spans, dtype=np.int32).reshape(-1, 3)
  W = len(spans)
  sp = np.concatenate([spans.reshape(-1), np.zeros(3, np.int32)])
  max_len = max([len(l) for l in labels] + [0]) if max_label_len is None else max_label_len
  log_prob = np.full(B + 1, 7.0)
  log_conf = np.full(W + 1, 7.0)
  status = np.full(B + 1, -7, dtype=np.int32)
  ws = np.zeros(lib.st_ctc_word_conf_ws(B, T, max_len, B + W) // 8 + 1, dtype=np.float64)
  _lib.call('st_ctc_word_conf_host', _p(logits), B, T, Cc, _p(ids), _p(offs), _p(np.asarray(seq_lens, dtype=np.int32)), max_len,
            space_id, _p(sp), W, _p(log_prob), _p(log_conf), _p(status), _p(ws), ws.nbytes)
  assert log_prob[-1] == 7.0 and log_conf[-1] == 7.0 and status[-1] == -7          # nothing written past the outputs
  return log_prob[:B], log_conf[:W], status[:B], spans


def dispatch_batch(rng, l_max, l_lo, frames, planted):
  """Five utterances of one dispatch: the longest label it holds, the shortest that needs it, a short one, an empty one and
  one that does not fit its frames; ragged lengths; random logits of scale 0.05, 1 or 4, or planted-path logits."""
  xs, labs = [], []
  for L, T in ((l_max, frames), (l_lo, int(rng.integers(frames // 2, frames))), (int(rng.integers(1, 12)), int(rng.integers(20, frames))),
               (0, int(rng.integers(0, 30)))):
    kw = dict(word_len=(1, max(6, L // 8)), edge_space_prob=0.3, double_space_prob=0.1)
    lab = CO.random_word_labels(rng, L, C, SPACE, repeat_prob=0.15, **kw)
    T = max(T, AO.min_frames(lab) + int(rng.integers(0, 3)))
    if T > frames:                                        # too many repeats for this frame count: thin them out
      lab = CO.random_word_labels(rng, L, C, SPACE, repeat_prob=0.0, word_len=kw['word_len'])
      T = max(min(T, frames), AO.min_frames(lab))
    assert len(lab) == L and AO.min_frames(lab) <= T <= frames
    if planted and T > 0:
      x = AO.planted_logits(rng, lab, T, C)[0]
    else:
      x = AO.random_logits(rng, T, C, scale=float(rng.choice([0.05, 1.0, 4.0])))
    xs.append(x)
    labs.append(lab)
  lab = CO.random_word_labels(rng, min(l_max, 40), C, SPACE, repeat_prob=0.5)       # does not fit: one frame short
  xs.append(AO.random_logits(rng, AO.min_frames(lab) - 1, C))
  labs.append(lab)
  return xs, labs


@functools.lru_cache(maxsize=None)
def dispatch_cases(planted):
  """The dispatch batches, made once: [(logits [B, frames, C], labels, seq_lens, per-utterance logits)]."""
  rng = np.random.default_rng(70 + int(planted))
  out, l_lo = [], 0
  for l_max, frames in DISPATCH:
    xs, labs = dispatch_batch(rng, l_max, l_lo + 1 if l_lo else 1, frames, planted)
    l_lo = l_max
    logits, lens = AO.pad_batch(xs, frames)
    out.append((logits, labs, lens, xs))
  return out


def check_against_oracle(xs, labs, log_prob, log_conf, status, spans, space_id=SPACE):
  """A batch result against the oracle -> (largest |d log_prob|, largest |d log_conf|) over the utterances that fit."""
  worst = [0.0, 0.0]
  for b, (x, lab) in enumerate(zip(xs, labs)):
    mine = log_conf[spans[:, 0] == b]
    ref = CO.word_conf64(x, lab, space_id)
    if ref is None:
      assert status[b] != 0 and log_prob[b] == -np.inf and np.isnan(mine).all()
      continue
    assert status[b] == 0 and len(mine) == len(ref['log_conf'])
    assert (mine <= 0.0).all()
    for got, want, k in [(np.array([log_prob[b]]), np.array([ref['log_prob']]), 0), (mine, ref['log_conf'], 1)]:
      inf = np.isinf(want)
      assert (got[inf] == want[inf]).all()
      if (~inf).any():
        worst[k] = max(worst[k], float(np.abs(got[~inf] - want[~inf]).max()))
  return worst


# ---- the oracle against brute force -------------------------------------------------------------------------------------------

def _small_cases():
  """Random labels over two letters, a space (2) and the blank (3), T in 3..7, with leading, trailing and double spaces."""
  rng = np.random.default_rng(5)
  cases = []
  fixed = [[0], [2, 0], [0, 2], [0, 2, 1], [0, 2, 2, 1], [2, 0, 1, 2], [0, 0, 2, 0], [1, 2, 1, 2, 1], [0, 1, 1], [2, 2, 0]]
  while len(cases) < 36:
    T = int(rng.integers(3, 8))
    if len(cases) < len(fixed):
      lab = fixed[len(cases)]
    else:
      lab = CO.random_word_labels(rng, int(rng.integers(1, 5)), 4, 2, word_len=(1, 2), repeat_prob=0.3, edge_space_prob=0.4,
                                  double_space_prob=0.3)
    if AO.min_frames(lab) > T or not CO.split_words(lab, 2):
      continue
    cases.append((AO.random_logits(rng, T, 4, scale=float(rng.choice([0.3, 1.0, 3.0]))), lab))
  return cases


def test_oracle_equals_the_enumeration_and_sees_double_counting():
  cases = _small_cases()
  assert len(cases) >= 30
  assert any(l[0] == 2 for _, l in cases) and any(l[-1] == 2 for _, l in cases)
  assert any(any(a == b == 2 for a, b in zip(l, l[1:])) for _, l in cases)
  worst, n_words, live_off = 0.0, 0, 0
  for x, lab in cases:
    ref = CO.word_conf64(x, lab, 2)
    live = CO.word_conf64(x, lab, 2, live_blanks=True)
    p = CO.brute_force(x, lab, 2)
    assert abs(ref['log_prob'] - p) <= 1e-12
    for j, w in enumerate(ref['words']):
      star = CO.brute_force(x, lab, 2, word=w)
      worst = max(worst, abs(ref['ln_star'][j] - star))
      assert abs(ref['ln_star'][j] - star) <= 1e-12, (lab, w)
      assert star >= p - 1e-12                                  # every alignment of the label lies inside the * event
      assert abs(ref['log_conf'][j] - min(0.0, p - star)) <= 1e-12
      live_off += abs(live['ln_star'][j] - star) > 1e-6
      n_words += 1
  assert live_off > 0                                           # blanks left alive beside * count paths twice: seen
  print('oracle against enumeration: {} labels, {} words, largest difference {:.3g}; the live-blank lattice is off on {}'.format(
      len(cases), n_words, worst, live_off))


# ---- properties of the oracle --------------------------------------------------------------------------------------------------

def test_confidence_is_a_probability():
  rng = np.random.default_rng(6)
  for _ in range(20):
    lab = CO.random_word_labels(rng, int(rng.integers(1, 30)), C, SPACE, edge_space_prob=0.3, double_space_prob=0.2)
    x = AO.random_logits(rng, AO.min_frames(lab) + int(rng.integers(0, 40)), C, scale=float(rng.choice([0.05, 1.0, 4.0])))
    ref = CO.word_conf64(x, lab, SPACE)
    assert (ref['log_conf'] <= 0.0).all() and (ref['ln_star'] >= ref['log_prob'] - 1e-10).all()


def test_a_certain_word_has_confidence_one():
  rng = np.random.default_rng(7)
  lab = [3, 4, 4, 5, 3]
  path = AO.random_alignment(rng, lab, 17)
  x = np.full((17, C), -np.inf, dtype=np.float32)
  for t, u in enumerate(path):
    x[t, lab[u // 2] if u & 1 else C - 1] = rng.standard_normal()
  x[:, SPACE] = rng.standard_normal(17)                        # the space stays possible: it lies outside the word's event
  ref = CO.word_conf64(x, lab, SPACE)
  assert ref['log_prob'] < -1.0 and abs(ref['log_conf'][0]) <= 1e-12
  lp, lc, st, _ = host_conf(x[None], [lab], [17])
  assert st[0] == 0 and abs(lc[0]) <= 1e-12 and abs(lp[0] - ref['log_prob']) <= GATE


def test_a_wrong_letter_lowers_its_word_alone():
  rng = np.random.default_rng(8)
  lab = [1, 2, 3, SPACE, 4, 5, 6, 7, SPACE, 8, 9]
  x = AO.planted_logits(rng, lab, 40, C)[0]
  ref = CO.word_conf64(x, lab, SPACE)
  wrong = list(lab)
  wrong[5] = 20
  bad = CO.word_conf64(x, wrong, SPACE)
  assert bad['log_conf'][1] < ref['log_conf'][1] - 1.0
  assert abs(bad['ln_star'][1] - ref['ln_star'][1]) <= 1e-12      # the * lattice does not see the word's letters
  lp, lc, st, _ = host_conf(np.stack([x, x]), [lab, wrong], [40, 40])
  assert lc[4] < lc[1] - 1.0 and np.abs(lc - np.concatenate([ref['log_conf'], bad['log_conf']])).max() <= GATE


# ---- the host form against the oracle --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('planted', [False, True], ids=['random', 'planted'])
def test_host_form_against_oracle(planted):
  """Measured on the CPU, largest absolute differences over the ten dispatch batches:
  random logits   |d log_prob| 7.3e-12, |d log_conf| 1.7e-11;
  planted logits  |d log_prob| 5.0e-14, |d log_conf| 9.2e-14   (gate: 1e-9)."""
  worst = [0.0, 0.0]
  for logits, labs, lens, xs in dispatch_cases(planted):
    lp, lc, st, spans = host_conf(logits, labs, lens)
    assert st.tolist() == [0, 0, 0, 0, 1]
    w = check_against_oracle(xs, labs, lp, lc, st, spans)
    worst = [max(worst[0], w[0]), max(worst[1], w[1])]
  print('host form, {}: largest |d log_prob| {:.3g}, |d log_conf| {:.3g}'.format('planted' if planted else 'random', *worst))
  assert worst[0] <= GATE and worst[1] <= GATE


EDGES = [
    ('word at the start and at the end', [1, 2, SPACE, 3, 4], 20),
    ('single-letter words', [5, SPACE, 6, SPACE, 7], 14),
    ('one word, the whole label', [1, 2, 3, 4, 5, 6], 9),
    ('equal letters in a word and across a space', [1, 1, 2, SPACE, 2, SPACE, SPACE, 2, 2], 30),
    ('spaces at both ends', [SPACE, 1, 2, SPACE], 11),
    ('spaces alone', [SPACE, SPACE], 6),
]


def test_edge_cases():
  rng = np.random.default_rng(9)
  worst = [0.0, 0.0]
  for scale in (0.05, 1.0, 4.0):
    xs, labs = [], []
    for _, lab, T in EDGES:
      labs.append(lab)
      xs.append(AO.random_logits(rng, T, C, scale))
    for _, lab, _ in EDGES:                                # the same labels on exactly the frames they need
      labs.append(lab)
      xs.append(AO.random_logits(rng, AO.min_frames(lab), C, scale))
    logits, lens = AO.pad_batch(xs)
    lp, lc, st, spans = host_conf(logits, labs, lens)
    assert (st == 0).all() and len(lc) == 2 * sum(len(CO.split_words(l, SPACE)) for _, l, _ in EDGES)
    w = check_against_oracle(xs, labs, lp, lc, st, spans)
    worst = [max(worst[0], w[0]), max(worst[1], w[1])]
  assert worst[0] <= GATE and worst[1] <= GATE
  # a class count below the vocabulary's, and another space id
  lab = [0, 1, 2, 1, 2, 0]
  x = AO.random_logits(rng, 12, 4, 1.0)
  lp, lc, st, spans = host_conf(x[None], [lab], [12], space_id=2)
  w = check_against_oracle([x], [lab], lp, lc, st, spans, space_id=2)
  assert len(lc) == 3 and max(w) <= GATE


def test_impossible_label_and_single_infinite_logits():
  rng = np.random.default_rng(10)
  lab = [1, 2, SPACE, 3]
  x = AO.random_logits(rng, 12, C, 1.0)
  dead = x.copy()
  dead[:, 2] = -np.inf                                         # the letter 2 can never be emitted: P(l) = 0
  some = x.copy()
  some[3, 2] = some[5, C - 1] = some[7, SPACE] = -np.inf       # single frames: P(l) stays positive
  lp, lc, st, spans = host_conf(np.stack([dead, some]), [lab, lab], [12, 12])
  assert st.tolist() == [0, 0] and lp[0] == -np.inf and (lc[:2] == -np.inf).all()
  ref = CO.word_conf64(dead, lab, SPACE)
  assert ref['log_prob'] == -np.inf and (ref['log_conf'] == -np.inf).all()
  assert max(check_against_oracle([dead, some], [lab, lab], lp, lc, st, spans)) <= GATE and np.isfinite(lc[2:]).all()


def test_refusals_arguments_and_unsafe_spans():
  from speecht_amd import _lib
  rng = np.random.default_rng(11)
  labs = [[1, 2, SPACE, 3], [4, 4, 4], []]
  xs = [AO.random_logits(rng, 9, C), AO.random_logits(rng, 4, C), AO.random_logits(rng, 0, C)]
  logits, lens = AO.pad_batch(xs)
  lp, lc, st, spans = host_conf(logits, labs, lens)
  assert st.tolist() == [0, 1, 0] and lp[1] == -np.inf and lp[2] == 0.0 and np.isnan(lc[2]) and np.isfinite(lc[:2]).all()
  # no words at all
  lp0, lc0, st0, _ = host_conf(logits, [[], [SPACE], []], lens)
  assert len(lc0) == 0 and st0.tolist() == [0, 0, 0] and abs(lp0[0] - AO.log_softmax64(xs[0])[:, C - 1].sum()) <= GATE
  # spans that are not word runs: unspecified values, but the call returns and stays inside its outputs
  wild = [(0, 0, 4), (0, 2, 3), (0, 3, 2), (0, -1, 2), (0, 0, 5), (7, 0, 1), (-1, 0, 1), (1, 0, 1), (2, 0, 1)]
  _, lcw, _, _ = host_conf(logits, labs, lens, spans=wild)
  assert np.isnan(lcw[2:]).all()
  # more than 30 classes, a space id outside the labels: errors
  with pytest.raises(_lib.SpeechtHipError):
    host_conf(np.zeros((1, 5, 31), np.float32), [[1]], [5])
  with pytest.raises(_lib.SpeechtHipError):
    host_conf(logits, labs, lens, space_id=C - 1)
  assert _lib.load().st_ctc_word_conf_ws(2, 10, 512, 2) == 0 and _lib.load().st_ctc_word_conf_ws(2, 10, 5, 1) == 0
  assert _lib.load().st_ctc_word_conf_ws(2, 10, 5, 9) == 2 * 10 * 256 + 9 * 8 + 512


# ---- the word splitter and the output formats ------------------------------------------------------------------------------------

def test_word_runs_and_formats():
  from speecht_amd import alignment, vocabulary
  S = vocabulary.SPACE_ID
  assert S == SPACE
  for ids in ([], [S], [S, S], [1], [1, S], [S, 1], [1, 2, S, S, 3], [S, 1, S, 2, 3, S], [1, S, 2, S, 3]):
    assert alignment.word_runs(ids) == CO.split_words(ids, S)
  assert alignment.word_runs([1, 2, S, S, 3]) == [(0, 2), (4, 5)]
  assert alignment.word_runs([0, 1, 0], space_id=1) == [(0, 1), (2, 3)]
  ids = vocabulary.sentence_to_ids(' so it  is ')
  spans = np.array([[2 * k, 2 * k + 1] for k in range(len(ids))])
  assert [w for w, _, _ in alignment.word_spans(ids, spans)] == ['so', 'it', 'is']
  assert alignment.word_spans(ids, spans)[2] == ('is', 16, 19)
  conf = dict(log_prob=-12.5, words=[0.91, 0.5, 0.123456789])
  assert alignment.confident_words(ids, conf['words']) == [dict(word='so', confidence=0.91), dict(word='it', confidence=0.5),
                                                           dict(word='is', confidence=0.123457)]
  with pytest.raises(ValueError):
    alignment.confident_words(ids, [0.5])
  entry = dict(path='a.flac', seconds=2.0, sample_rate=16000, text=' so it  is ', ids=ids, spans=spans, score=-3.0, frames=30)
  plain = alignment.result_json(entry)
  assert set(plain) == {'path', 'seconds', 'text', 'score', 'score_per_frame', 'words'}
  assert all(set(w) == {'word', 'start', 'end'} for w in plain['words'])
  timed = alignment.result_json(dict(entry, confidence=conf), chars=True)
  assert timed['log_prob'] == -12.5 and [w['confidence'] for w in timed['words']] == [0.91, 0.5, 0.123457]
  assert [{k: w[k] for k in ('word', 'start', 'end')} for w in timed['words']] == plain['words']
  assert len(timed['chars']) == len(ids) and json.loads(json.dumps(timed)) == timed
  bare = alignment.result_json(dict(entry, spans=None, score=None, confidence=conf))
  assert bare['words'] == alignment.confident_words(ids, conf['words']) and bare['log_prob'] == -12.5 and 'score' not in bare
  out = io.StringIO()
  alignment.print_words(entry, file=out)
  alignment.print_words(dict(entry, confidence=conf), file=out)
  alignment.print_words(dict(entry, spans=None, confidence=conf), file=out)
  lines = [l.split('\t') for l in out.getvalue().splitlines()]
  assert [len(l) for l in lines] == [4] * 3 + [5] * 6
  assert lines[3][:4] == lines[0] and lines[3][4] == '0.9100' and lines[8] == ['a.flac', '-', '-', 'is', '0.1235']
