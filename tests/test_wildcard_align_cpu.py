"""The wildcard label and the per-label fit of the forced alignment, without a GPU: the float64 oracle
(tests/wildcard_align_oracle.py) against brute-force path enumeration, both host forms (st_ctc_align_wild_host,
st_ctc_align_long_wild_host -- the recursion the kernels share through csrc/ctc_align_core.h) against the oracle and against the
plain host forms, the argument validation of the C ABI, the planted experiment the wildcard exists for, the fit, and the
transcript / CLI surface.

The planted experiment (`planted_gap_case`): 12 labels over 40 frames, 50 frames spelling 15 other labels the transcript leaves
out, 12 labels over 40 frames; the reference for every transcribed span is what its part gets when aligned alone.  Measured on
the 40 trials of seed 2024, float64 oracle and host form alike: with a wildcard at bias -1.0 (and -0.5) 39 of 40 trials exact
and none more than 2 frames off; at bias 0 only 11 of 40 exact, up to 4 frames off (the tie rule hands frames that the greedy
reading agrees with to the wildcard); the plain aligner on the two parts' labels errs by 18.7 frames (largest span edge error
per trial, mean over the trials)."""
import ctypes
import importlib.machinery
import importlib.util
import itertools
import os

import numpy as np
import pytest

from tests import align_oracle as AO
from tests import wildcard_align_oracle as WO
from tests import wildcard_align_util as WU
from tests.align_long_util import host_align_long
from tests.test_align_cpu import host_align

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_FLAC = os.path.join(ROOT, 'tests', 'golden', '1089-134686-0037.flac')
ST_EINVAL = -1
BIASES = (0.0, -0.5, -1.0, -3.25)


def _cli():
  loader = importlib.machinery.SourceFileLoader('speecht_cli_wild', os.path.join(ROOT, 'speecht-cli'))
  spec = importlib.util.spec_from_loader('speecht_cli_wild', loader)
  cli = importlib.util.module_from_spec(spec)
  loader.exec_module(cli)
  return cli


def _p(a):
  return ctypes.c_void_p(a.ctypes.data)


def _random_wild_labels(rng, L, C):
  """L random ids with repeats and wildcards sprinkled in, never two of them in a row."""
  W = WO.wild_id(C)
  lab = []
  for l in AO.random_labels(rng, L, C):
    lab.append(W if rng.random() < 0.25 and (not lab or lab[-1] != W) else l)
  return lab


# ---- the oracle ---------------------------------------------------------------------------------------------------------------

def test_oracle_matches_brute_force():
  """Every monotone state sequence of a tiny lattice (T <= 7, L <= 3): the oracle returns the best score, and its path is one of
  those that reach it.  Wildcard first, last, alone, between equal ids, and every other arrangement of 0 .. 3 labels."""
  C = 4
  W = WO.wild_id(C)
  rng = np.random.default_rng(1)
  shapes = [[W], [W, 0], [0, W], [1, W, 1], [W, 1, 1], [1, 1, W], [W, 2, W], [0, W, 1], []]
  shapes += [list(l) for n in (1, 2, 3) for l in itertools.product((0, 2, W), repeat=n)
             if not any(a == W and b == W for a, b in zip(l, l[1:]))]
  checked = 0
  for lab in shapes:
    for T in range(max(AO.min_frames(lab), 1), 8):
      for bias in (0.0, -0.7):
        x = AO.random_logits(rng, T, C, scale=2.0)
        ref = WO.align_wild64(x, lab, bias)
        brute = WO.brute_force(x, lab, bias)
        assert ref is not None and brute is not None
        states, spans, score = ref
        assert abs(score - brute[0]) <= 1e-12 * max(abs(score), 1.0), (lab, T, bias)
        assert AO.is_valid_alignment(states, lab)
        assert abs(WO.path_score_wild64(x, states, lab, bias) - score) <= 1e-12 * max(abs(score), 1.0)
        checked += 1
    if AO.min_frames(lab) > 0:
      assert WO.align_wild64(AO.random_logits(rng, AO.min_frames(lab) - 1, C), lab, -1.0) is None
      assert WO.brute_force(AO.random_logits(rng, AO.min_frames(lab) - 1, C), lab, -1.0) is None
  assert checked > 300
  # without a wildcard: align_oracle.align64, whatever the bias
  for _ in range(20):
    lab = AO.random_labels(rng, int(rng.integers(0, 6)), C)
    x = AO.random_logits(rng, AO.min_frames(lab) + int(rng.integers(1, 6)), C)
    a, b = AO.align64(x, lab), WO.align_wild64(x, lab, -2.0)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2] == b[2]
  for bad in ([W, W], [0, W, W, 1], [3], [-1]):
    with pytest.raises(ValueError):
      WO.align_wild64(AO.random_logits(rng, 9, C), bad, -1.0)
  for bias in (0.5, np.nan, -np.inf):
    with pytest.raises(ValueError):
      WO.align_wild64(AO.random_logits(rng, 9, C), [W], bias)


def test_oracle_tie_rules_with_bias_zero():
  """bias = 0 on logits whose greedy reading spells the labels: the wildcard ties with a label on every such frame, and the
  tie rule (stay, then advance, then skip; decided at the later frame) hands those frames to the wildcard that FOLLOWS."""
  C = 4
  W = WO.wild_id(C)
  x = np.full((6, C), -9.0, dtype=np.float32)
  for t, c in enumerate([0, 0, 0, 1, 1, 1]):
    x[t, c] = 9.0
  # "0 W": every frame ties; the back-trace from the end stays in W as long as it can, label 0 keeps frame 0 only
  states, spans, score = WO.align_wild64(x, [0, W], 0.0)
  assert states.tolist() == [0, 1, 1, 1, 1, 1] and spans.tolist() == [[0, 1], [1, 6]]
  # "W 1": the wildcard comes first and gives way at the first frame that reads 1 (advance needs a strictly better score)
  states, spans, score = WO.align_wild64(x, [W, 1], 0.0)
  assert states.tolist() == [0, 0, 0, 1, 1, 1]
  # a negative bias gives the label every frame that reads it, and the wildcard the frames that read something else
  states, _, _ = WO.align_wild64(x, [0, W], -1.0)
  assert states.tolist() == [0, 0, 0, 1, 1, 1]
  states, _, _ = WO.align_wild64(x[:3], [0, W], -1.0)                 # nothing else is read: the one frame a label must have
  assert states.tolist() == [0, 0, 1]
  # all-zero logits: everything ties, the oracle and both host forms take the same path
  zero = np.zeros((9, C), dtype=np.float32)
  for lab in ([W], [0, W, 0], [W, 1, W], [2, 2, W]):
    ref = WO.align_wild64(zero, lab, 0.0)
    spans, states, _, status, _ = WU.host_align_wild(zero[None], [lab], [9], 0.0)
    assert status[0] == 0 and (states[0] == ref[0]).all() and (spans[0] == ref[1]).all()
    assert (WU.host_align_long_wild(zero, lab, 0.0)[0] == ref[1]).all()


# ---- the host forms -------------------------------------------------------------------------------------------------------------

def test_library_exports_the_wildcard_entry_points():
  from speecht_amd import _lib
  lib = _lib.load()
  header = open(os.path.join(ROOT, 'include', 'speecht_hip.h')).read()
  for name in ('st_ctc_align_wild_f32', 'st_ctc_align_wild_host', 'st_ctc_align_long_wild_f32', 'st_ctc_align_long_wild_host'):
    assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS and name + '(' in header
  sig = _lib._SIGNATURES
  for plain, wild in (('st_ctc_align_f32', 'st_ctc_align_wild_f32'), ('st_ctc_align_host', 'st_ctc_align_wild_host'),
                      ('st_ctc_align_long_f32', 'st_ctc_align_long_wild_f32'), ('st_ctc_align_long_host', 'st_ctc_align_long_wild_host')):
    assert len(sig[wild][1]) == len(sig[plain][1]) + 2 and ctypes.c_double in sig[wild][1]


@pytest.mark.parametrize('planted', [False, True], ids=['random', 'planted'])
def test_host_forms_against_the_oracle(planted):
  """Both host forms on random and planted logits: the oracle's path (planted: the planted one), the accuracy conditions of
  tests/test_align_cpu.py, the fit; the two host forms agree bit for bit."""
  rng = np.random.default_rng(20 + int(planted))
  worst = [0.0, 0.0]
  for case in range(60):
    C = int(rng.choice([2, 3, 5, 17, 29, 31]))
    W = WO.wild_id(C)
    bias = float(rng.choice(BIASES))
    lab = _random_wild_labels(rng, int(rng.integers(0, 40)), C)
    T = max(AO.min_frames(lab) + int(rng.integers(0, 60)), 1)
    if planted:
      # plant a path of ordinary labels; the wildcards stand where labels of it are left out of the transcript
      full = [l if l != W else int(rng.integers(C - 1)) for l in lab]
      x, path = AO.planted_logits(rng, full, max(T, AO.min_frames(full)), C)
      T = x.shape[0]
    else:
      x = AO.random_logits(rng, T, C, scale=float(rng.choice([0.05, 1.0, 3.0, 10.0])))
    spans, states, score, status, fit = WU.host_align_wild(x[None], [lab], [T], bias)
    r = WU.check_wild_utterance(x, lab, spans[0], states[0], score[0], status[0], fit[0], bias, T)
    worst = [max(worst[0], r[0]), max(worst[1], r[1])]
    ref = WO.align_wild64(x, lab, bias)
    if planted:                                                      # a clear optimum: the oracle's own path, frame by frame
      assert (ref[0] == states[0]).all(), case
    long = WU.host_align_long_wild(x, lab, bias)
    assert (long[0] == spans[0]).all() and np.float32(long[1]) == score[0] and long[2] == 0
    assert (WU.bits(long[3]) == WU.bits(fit[0])).all()
  print('host forms, {}: largest ratio to the bound: path {:.3g}, score {:.3g}'.format('planted' if planted else 'random', *worst))


def test_without_a_wildcard_the_plain_host_forms():
  """No wildcard among the labels: spans, states, the score's bits and the status of st_ctc_align_host and
  st_ctc_align_long_host, for any bias -- refused utterances and ragged batches included."""
  rng = np.random.default_rng(22)
  for case in range(25):
    C = int(rng.choice([2, 5, 29, 31]))
    B = 4
    labs = [AO.random_labels(rng, int(rng.integers(0, 50)), C) for _ in range(B)]
    Ts = [max(AO.min_frames(l) + int(rng.integers(-1, 30)), 0) for l in labs]
    xs = [AO.random_logits(rng, t, C, scale=float(rng.choice([0.05, 1.0, 4.0]))) for t in Ts]
    logits, lens = AO.pad_batch(xs)
    plain = host_align(logits, labs, lens)
    for bias in (0.0, -1.0, -7.5):
      wild = WU.host_align_wild(logits, labs, lens, bias)
      assert (wild[3] == plain[3]).all() and (wild[1] == plain[1]).all()
      assert (wild[2].view(np.int32) == plain[2].view(np.int32)).all()
      assert all((a == b).all() for a, b in zip(wild[0], plain[0]))
      assert all(np.isnan(f).all() == (s != 0) or len(f) == 0 for f, s in zip(wild[4], wild[3]))
    b = int(np.argmax(Ts))
    if Ts[b] > 0:
      p = host_align_long(xs[b], labs[b])
      w = WU.host_align_long_wild(xs[b], labs[b], -1.0)
      assert WU.same_long(w[:3] + (np.zeros(0),), p + (np.zeros(0),))
      assert WU.same_long(WU.host_align_long_wild(xs[b], labs[b], -1.0, want_fit=False)[:3] + (np.zeros(0),), p + (np.zeros(0),))


def test_one_refused_utterance_leaves_its_neighbours_alone():
  rng = np.random.default_rng(23)
  C = 29
  W = WO.wild_id(C)
  labs = [[W] + AO.random_labels(rng, 20, C, 0.1), [W] + AO.random_labels(rng, 24, C, 0.0) + [W], [3, W, 3], []]
  xs = [AO.random_logits(rng, 60, C), AO.random_logits(rng, 25, C), AO.random_logits(rng, 3, C), AO.random_logits(rng, 0, C)]
  logits, lens = AO.pad_batch(xs)
  spans, states, score, status, fit = WU.host_align_wild(logits, labs, lens, -1.0)
  # the second transcript has 26 labels once its wildcards count: one more than its frames
  assert status.tolist() == [0, 1, 0, 0] and (spans[1] == -1).all() and score[1] == -np.inf and np.isnan(fit[1]).all()
  assert (states[1] == -2).all() and spans[2].tolist() == [[0, 1], [1, 2], [2, 3]]
  for b in (0, 2):
    WU.check_wild_utterance(xs[b], labs[b], spans[b], states[b], score[b], status[b], fit[b], -1.0, logits.shape[1])
    alone = WU.host_align_wild(logits[b:b + 1], [labs[b]], lens[b:b + 1], -1.0, max_label_len=26)
    assert (alone[0][0] == spans[b]).all() and (WU.bits(alone[4][0]) == WU.bits(fit[b])).all()
  # the same transcript without its wildcards fits: the wildcards count in the fit rule
  assert WU.host_align_wild(logits[1:2], [labs[1][1:-1]], lens[1:2], -1.0)[3][0] == 0
  assert WU.host_align_long_wild(xs[1], labs[1], -1.0)[2] == 1 and np.isnan(WU.host_align_long_wild(xs[1], labs[1], -1.0)[3]).all()
  assert WU.host_align_long_wild(xs[1][:25], labs[1][:-1], -1.0)[2] == 0


def test_abi_argument_validation():
  from speecht_amd import _lib
  from speecht_amd._lib import Tensor3
  lib = _lib.load()
  rng = np.random.default_rng(24)
  C, T = 5, 12
  W = WO.wild_id(C)
  x = AO.random_logits(rng, T, C)
  ok = [0, W, 1]
  assert WU.host_align_wild(x[None], [ok], [T], -1.0, check=False) == 0
  assert WU.host_align_long_wild(x, ok, -1.0, check=False) == 0
  for bias in (0.5, 1e-300, float('nan'), float('inf'), float('-inf')):
    assert WU.host_align_wild(x[None], [ok], [T], bias, check=False) == ST_EINVAL and b'wildcard_bias' in lib.st_last_error()
    assert WU.host_align_long_wild(x, ok, bias, check=False) == ST_EINVAL and b'wildcard_bias' in lib.st_last_error()
  for bad in ([W, W], [0, W, W], [0, W, 1, W, W]):
    assert WU.host_align_wild(x[None], [bad], [T], -1.0, check=False) == ST_EINVAL and b'adjacent' in lib.st_last_error()
    assert WU.host_align_long_wild(x, bad, -1.0, check=False) == ST_EINVAL and b'adjacent' in lib.st_last_error()
  # a wildcard that ends one utterance and one that begins the next are not adjacent
  assert WU.host_align_wild(np.stack([x, x]), [[0, W], [W, 1]], [T, T], -1.0, check=False) == 0
  for bad in ([W + 1], [-1], [0, 99]):
    assert WU.host_align_wild(x[None], [bad], [T], -1.0, check=False) == ST_EINVAL and b'label id' in lib.st_last_error()
    assert WU.host_align_long_wild(x, bad, -1.0, check=False) == ST_EINVAL
  # classes = 32 leaves the wildcard no slot
  x32 = AO.random_logits(rng, T, 32)
  assert WU.host_align_wild(x32[None], [[0, 1]], [T], -1.0, check=False) == ST_EINVAL and b'2..31' in lib.st_last_error()
  assert WU.host_align_long_wild(x32, [0, 1], -1.0, check=False) == ST_EINVAL and b'2..31' in lib.st_last_error()
  assert WU.host_align_wild(AO.random_logits(rng, T, 31)[None], [[0, 31]], [T], -1.0, check=False) == 0
  # the device forms refuse the same before anything is launched: no device is touched
  xp = np.zeros((1, T, 32), dtype=np.float32)
  ids, offs, lens = np.zeros(4, dtype=np.int32), np.array([0, 2], dtype=np.int32), np.array([T], dtype=np.int32)
  spans, states, fit = np.zeros((4, 2), dtype=np.int32), np.zeros((1, T), dtype=np.int32), np.zeros(4)
  score, status = np.zeros(1, dtype=np.float32), np.zeros(1, dtype=np.int32)
  need = lib.st_ctc_align_ws(1, T, 2)
  ws = np.zeros(need // 8 + 1, dtype=np.float64)

  def device(classes=C, bias=-1.0, L=2, nbytes=need, ids_p=_p(ids)):
    d = Tensor3(xp.ctypes.data, 1, T, classes, 0, T, 32)
    return lib.st_ctc_align_wild_f32(ctypes.byref(d), ids_p, _p(offs), _p(lens), L, bias, _p(spans), _p(states), _p(score), _p(status),
                                     _p(fit), _p(ws), nbytes, None)

  assert device(classes=32) == ST_EINVAL and b'2..31' in lib.st_last_error()
  assert device(bias=0.25) == ST_EINVAL and device(bias=float('nan')) == ST_EINVAL and b'wildcard_bias' in lib.st_last_error()
  assert device(L=512) == ST_EINVAL and device(nbytes=need - 1) == ST_EINVAL and device(ids_p=None) == ST_EINVAL
  dscore = np.zeros(1)
  need_long = lib.st_ctc_align_long_ws(T, 2)
  wl = np.zeros(need_long // 8 + 1, dtype=np.float64)

  def device_long(classes=C, bias=-1.0, nbytes=need_long, pitch=32):
    return lib.st_ctc_align_long_wild_f32(_p(xp), T, classes, pitch, _p(ids), 2, bias, _p(spans), _p(dscore), _p(status), _p(fit),
                                          _p(wl), nbytes, None)

  assert device_long(classes=32) == ST_EINVAL and b'2..31' in lib.st_last_error()
  assert device_long(bias=1.0) == ST_EINVAL and device_long(bias=float('-inf')) == ST_EINVAL
  assert device_long(nbytes=need_long - 1) == ST_EINVAL and device_long(pitch=4) == ST_EINVAL


# ---- what the wildcard is for ---------------------------------------------------------------------------------------------------

def test_planted_gap_on_the_host_form():
  """The experiment of the module text.  First the float64 oracle alone meets the conditions, then the host form:
  every transcribed span within 2 frames of the span its part gets alone, in every trial; at least 36 of 40 trials exact; the
  wildcard's span inside the left-out stretch +- 3 frames; the plain aligner errs by more than 10 frames on average."""
  for form in ('oracle', 'host'):
    rng = np.random.default_rng(2024)
    exact, plain_err = 0, []
    for trial in range(40):
      x, l1, l2, g0, g1 = WO.planted_gap_case(rng)
      C, T = x.shape[1], x.shape[0]
      want = np.concatenate([AO.align64(x[:g0], l1)[1], AO.align64(x[g1:], l2)[1] + g1])
      lab = l1 + [WO.wild_id(C)] + l2
      if form == 'oracle':
        spans = WO.align_wild64(x, lab, -1.0)[1]
        plain = AO.align64(x, l1 + l2)[1]
      else:
        spans = WU.host_align_wild(x[None], [lab], [T], -1.0)[0][0]
        plain = host_align(x[None], [l1 + l2], [T])[0][0]
        assert (WU.host_align_long_wild(x, lab, -1.0)[0] == spans).all()
      got = np.concatenate([spans[:len(l1)], spans[len(l1) + 1:]])
      off = int(np.abs(got - want).max())
      assert off <= 2, (form, trial, off)
      exact += off == 0
      a, b = spans[len(l1)]
      assert g0 - 3 <= a < b <= g1 + 3, (form, trial, a, b)
      plain_err.append(np.abs(plain - want).max())
    print('{}: {} of 40 exact; the plain aligner errs by {:.1f} frames on average'.format(form, exact, np.mean(plain_err)))
    assert exact >= 36 and np.mean(plain_err) > 10.0


# ---- the fit --------------------------------------------------------------------------------------------------------------------

def test_fit():
  """Exactly 0 for labels whose class is the row maximum on all their frames, bias x frames for wildcards, the float64 sum
  within 1e-9 relative elsewhere, NaN for a refused utterance, and nothing written with fit = null."""
  rng = np.random.default_rng(25)
  C = 29
  W = WO.wild_id(C)
  # planted at a boost that makes the planted class the row maximum on every frame
  lab = AO.random_labels(rng, 30, C, 0.2)
  x, path = AO.planted_logits(rng, lab, 120, C, boost=40.0)
  spans, states, score, status, fit = WU.host_align_wild(x[None], [lab], [120], -1.0)
  assert status[0] == 0 and [s for s in states[0]] == [u // 2 if u & 1 else -1 for u in path]
  assert (fit[0] == 0.0).all() and not np.signbit(fit[0]).any()
  # the same audio with three labels left out of the transcript and a wildcard in their place; and a wrong label
  cut = lab[:10] + [W] + lab[13:]
  cut[20] = (cut[20] + 1) % (C - 1)
  if cut[20] in (cut[19], cut[21]):
    cut[20] = (cut[20] + 1) % (C - 1)
  spans, states, score, status, fit = WU.host_align_wild(x[None], [cut], [120], -1.0)
  WU.check_fit(x, cut, spans[0], fit[0], -1.0)
  a, b = spans[0][10]
  assert fit[0][10] == -1.0 * (b - a) and b - a >= 3
  assert fit[0][20] < -30.0                                           # the wrong label: its frames say something else
  assert (np.delete(fit[0], [10, 20]) == 0.0).all()
  for bias in BIASES:
    sp, _, _, _, f = WU.host_align_wild(x[None], [cut], [120], bias)
    assert f[0][10] == np.float64(bias) * float(sp[0][10][1] - sp[0][10][0])
  # random logits: against the float64 sum (check_wild_utterance), both host forms the same bits
  for case in range(20):
    lab = _random_wild_labels(rng, int(rng.integers(1, 60)), C)
    T = AO.min_frames(lab) + int(rng.integers(0, 100))
    x = AO.random_logits(rng, T, C, scale=float(rng.choice([0.05, 1.0, 5.0])))
    spans, states, score, status, fit = WU.host_align_wild(x[None], [lab], [T], -0.5)
    WU.check_wild_utterance(x, lab, spans[0], states[0], score[0], status[0], fit[0], -0.5, T)
    assert (WU.bits(WU.host_align_long_wild(x, lab, -0.5)[3]) == WU.bits(fit[0])).all()
  # fit = null: the other outputs as with it
  with_fit = WU.host_align_wild(x[None], [lab], [T], -0.5)
  without = WU.host_align_wild(x[None], [lab], [T], -0.5, want_fit=False)
  assert (without[0][0] == with_fit[0][0]).all() and without[2][0] == with_fit[2][0] and (without[4][0] == 7.0).all()


def test_word_fits_and_gaps():
  from speecht_amd import alignment as A
  ids = A.transcript_ids('* the cat * sat', '*')
  assert ids == [A.WILDCARD, 27, 19, 7, 4, 27, 2, 0, 19, 27, A.WILDCARD, 27, 18, 0, 19]
  spans = [(3 * k, 3 * k + 2) for k in range(len(ids))]
  runs, stars = A.wild_word_runs(ids)
  assert runs == [(2, 5), (6, 9), (12, 15)] and stars == [0, 10]
  words, gaps = A.wild_word_spans(ids, spans)
  assert words == [('the', 6, 14), ('cat', 18, 26), ('sat', 36, 44)] and gaps == [(0, 2), (30, 32)]
  fit = np.zeros(len(ids))
  fit[[0, 10]] = -2.0                                                 # the wildcards' own fits belong to no word
  fit[6], fit[8] = -3.0, -6.0
  assert A.word_fits(ids, spans, fit) == [0.0, -1.5, 0.0]             # -9 nats over the 6 frames of c, a, t
  timed = A.timed_words(ids, spans, 16000, fit=fit)
  assert [w['word'] for w in timed] == ['the', 'cat', 'sat'] and [w['fit'] for w in timed] == [0.0, -1.5, 0.0]
  assert A.timed_words(ids, spans, 16000, gaps=True) == [dict(start=0.0, end=0.04), dict(start=0.6, end=0.64)]
  assert [c['char'] for c in A.timed_words(ids, spans, 16000, chars=True)] == list(' the cat  sat')
  # without a wildcard the helpers are word_runs / word_spans
  plain = A.transcript_ids('the cat')
  assert A.wild_word_runs(plain) == (A.word_runs(plain), [])
  assert A.wild_word_spans(plain, spans)[0] == A.word_spans(plain, spans)


# ---- transcripts and the CLI ----------------------------------------------------------------------------------------------------

def test_transcript_parsing():
  from speecht_amd import alignment as A
  from speecht_amd.transcription import TranscriptionError
  W, S = A.WILDCARD, 27
  assert A.WILDCARD == -1 and A.WILDCARD_TOKEN == '*' and A.WILDCARD_BIAS == -1.0
  assert A.transcript_ids('A * B', '*') == [0, S, W, S, 1]
  assert A.transcript_ids('* a', '*') == [W, S, 0] and A.transcript_ids('a *', '*') == [0, S, W]
  assert A.transcript_ids('*', '*') == [W] and A.transcript_ids('', '*') == []
  assert A.transcript_ids('a  *  b', '*') == [0, S, S, W, S, S, 1]           # double spaces stay
  assert A.transcript_ids('a * * b', '*') == [0, S, W, S, W, S, 1]           # a space between them: not adjacent
  assert A.transcript_ids('a <gap> b', '<GAP>') == [0, S, W, S, 1]
  assert A.transcript_ids("don't", '*') == A.transcript_ids("don't")
  # the token inside a word stays the vocabulary error it is; without the argument so does the token alone
  for text, token in (('a*b', '*'), ('a *b', '*'), ('a ** b', '*'), ('a * b', None), ('a # b', '*')):
    with pytest.raises(TranscriptionError):
      A.transcript_ids(text, token) if token else A.transcript_ids(text)
  for token in ('', 'a b', 'the', "don't"):
    with pytest.raises(ValueError):
      A.transcript_ids('a', token)
  # ends: a wildcard before and after, unless the text has one there
  assert A.transcript_ids('a b', '*', True) == [W, S, 0, S, 1, S, W]
  assert A.transcript_ids('* a b', '*', True) == [W, S, 0, S, 1, S, W]
  assert A.transcript_ids('a b *', '*', True) == [W, S, 0, S, 1, S, W]
  assert A.transcript_ids('', '*', True) == []


def test_engine_side_label_check():
  pytest.importorskip('torch')
  from speecht_amd import engine_decode as ED
  assert ED.WILDCARD == -1 and ED.WILDCARD_BIAS == -1.0
  assert ED.wildcard_ids('t', [0, ED.WILDCARD, 27], 29, True).tolist() == [0, 29, 27]
  assert ED.wildcard_ids('t', [], 29, True).tolist() == [] and ED.wildcard_ids('t', [ED.WILDCARD], 29, True).tolist() == [29]
  for bad in ([28], [29], [-2], [0, ED.WILDCARD, ED.WILDCARD]):
    with pytest.raises(ValueError):
      ED.wildcard_ids('t', bad, 29, True)
  with pytest.raises(ValueError, match='num_classes'):
    ED.wildcard_ids('t', [0], 32, True)


def test_cli_parsing():
  cli = _cli()
  _, flags = cli.parse(['align', 'a.flac'])
  assert not any(hasattr(flags, f) for f in ('wildcard', 'wildcard_ends', 'wildcard_bias', 'fit'))
  from speecht_amd import alignment as A
  assert A.wildcard_options(flags) == {}
  _, flags = cli.parse(['align', 'a.flac', '--wildcard'])
  assert flags.wildcard == '*' and flags.paths == ['a.flac']
  assert A.wildcard_options(flags) == dict(wildcard='*', ends=False, wildcard_bias=-1.0, fit=False)
  _, flags = cli.parse(['align', '--wildcard=<gap>', '--wildcard-bias', '-0.5', '--fit', 'a.flac'])
  assert A.wildcard_options(flags) == dict(wildcard='<gap>', ends=False, wildcard_bias=-0.5, fit=True)
  _, flags = cli.parse(['align', '--wildcard-ends', '--segment', 'a.flac'])
  assert A.wildcard_options(flags) == dict(wildcard='*', ends=True, wildcard_bias=-1.0, fit=False) and flags.segment
  _, flags = cli.parse(['align', '--fit', 'a.flac'])
  assert A.wildcard_options(flags) == dict(wildcard=None, ends=False, wildcard_bias=-1.0, fit=True)
  _, flags = cli.parse(['align', '--wildcard-bias', '0', 'a.flac'])
  assert A.wildcard_options(flags)['wildcard_bias'] == 0.0 and A.wildcard_options(flags)['wildcard'] == '*'
  for bad in (['--wildcard-bias', '0.5'], ['--wildcard-bias', 'nan'], ['--wildcard-bias', '-inf'], ['--wildcard=the'],
              ['--wildcard=']):
    with pytest.raises(SystemExit):
      cli.parse(['align'] + bad + ['a.flac'])
  with pytest.raises(SystemExit):
    cli.parse(['align', '--wildcard', GOLDEN_FLAC])                   # the bare flag took the path
  _, flags = cli.parse(['transcribe', 'a.flac'])
  assert not hasattr(flags, 'wildcard')


@pytest.mark.parametrize('flag', ['--wildcard', '--wildcard-ends', '--fit', '--wildcard-bias=-1'])
def test_cli_refuses_confidence_with_the_wildcard(flag, capsys):
  cli = _cli()
  with pytest.raises(SystemExit):
    cli.parse(['align', 'a.flac', '--confidence', flag])
  assert 'do not know the wildcard' in capsys.readouterr().err
  _, flags = cli.parse(['align', 'a.flac', '--confidence'])
  assert flags.confidence is True


def test_align_files_reports_problems_as_entries():
  """A `*` without the wildcard argument stays the vocabulary error it is; with it, a token glued to a word is one; confidence
  is refused (no device is needed: nothing is left to align)."""
  from speecht_amd.alignment import align_files
  res = align_files(None, [GOLDEN_FLAC, GOLDEN_FLAC], ['HE * SAID', 'HE *SAID'])
  assert all('outside the vocabulary' in r['error'] for r in res)
  res = align_files(None, [GOLDEN_FLAC], ['HE *SAID'], wildcard='*', fit=True)
  assert 'outside the vocabulary' in res[0]['error']
  with pytest.raises(ValueError, match='wildcard'):
    align_files(None, [GOLDEN_FLAC], ['HE SAID'], wildcard='*', confidence=True)
  with pytest.raises(ValueError, match='wildcard'):
    align_files(None, [GOLDEN_FLAC], ['HE SAID'], fit=True, confidence=True)
