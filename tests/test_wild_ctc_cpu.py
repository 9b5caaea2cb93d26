"""The wildcard CTC loss on the CPU: the float64 specification (tests/wild_ctc_oracle.py) against the plain oracle and against
torch autograd of a direct lattice, the case table's own claims (tests/wild_ctc_cases.py), partial_labels, the CLI flags, the
C ABI's three places, and the planted experiment whose numbers DESIGN.md quotes."""
import ctypes
import importlib.machinery
import importlib.util
import os

import numpy as np
import pytest

from tests import align_oracle as AO
from tests import ctc_cases as CC
from tests import wild_ctc_cases as WC
from tests import wild_ctc_oracle as WO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = WO.WILDCARD


def _cli():
  loader = importlib.machinery.SourceFileLoader('speecht_cli_wild_ctc', os.path.join(ROOT, 'speecht-cli'))
  spec = importlib.util.spec_from_loader('speecht_cli_wild_ctc', loader)
  cli = importlib.util.module_from_spec(spec)
  loader.exec_module(cli)
  return cli


# ---- the specification --------------------------------------------------------------------------------------------------------

def test_spec_equals_the_plain_oracle_without_a_wildcard():
  """Gradients to 1e-12 absolute; losses to 1e-12 absolute up to a loss of 1 and 1e-12 RELATIVE above it (the table's losses run
  into the hundreds, where 1e-12 absolute is a few ulps of a float64)."""
  from oracle import w2l_oracle as O
  rng = np.random.default_rng(1)
  worst = 0.0
  cases = [(u.logits, u.label) for name in ('wk1', 'wk3', 'wk1-C2', 'wk3-C31') for u in WC.batch_by_name(name).utterances if not u.wild]
  for _ in range(12):
    C = int(rng.choice([2, 3, 5, 29, 32]))
    label = AO.random_labels(rng, int(rng.integers(0, 9)), C, 0.3)
    x = AO.random_logits(rng, AO.min_frames(label) + int(rng.integers(0, 6)), C)
    if rng.random() < 0.3 and x.shape[0] and C > 2:
      x[rng.integers(x.shape[0]), [c for c in range(C - 1) if c not in label][:1]] = -np.inf
    cases.append((x, label))
  for x, label in cases:
    loss, grad = WO.ctc_loss_and_grad(x, label, -0.7)
    if x.shape[0] == 0:
      assert loss == 0.0
      continue
    with np.errstate(invalid='ignore', divide='ignore'):
      ref_loss, ref_grad = O.ctc_loss_and_grad(x.astype(np.float64)[:, None, :], [label], [x.shape[0]])
    worst = max(worst, abs(loss - ref_loss[0]) / max(1.0, abs(ref_loss[0])), float(np.max(np.abs(grad - ref_grad[:, 0]))))
  assert worst < 1e-12, worst


def _torch_lattice_loss(x, label, bias):
  """-ln sum over paths, in plain probabilities (tiny cases only), differentiable."""
  import torch
  T, C = x.shape
  blank = C - 1
  y = torch.softmax(x, dim=1)
  wild = np.exp(bias) * y[:, :blank].sum(dim=1)
  ext = [blank]
  for l in label:
    ext += [l, blank]
  em = lambda t, u: wild[t] if ext[u] == W else y[t, ext[u]]
  U = len(ext)
  zero = torch.zeros((), dtype=x.dtype)
  alpha = [em(0, u) if u < 2 else zero for u in range(U)]
  for t in range(1, T):
    new = []
    for u in range(U):
      s = alpha[u]
      if u >= 1:
        s = s + alpha[u - 1]
      if u >= 2 and u & 1 and ext[u] != ext[u - 2]:
        s = s + alpha[u - 2]
      new.append(s * em(t, u))
    alpha = new
  return -torch.log(alpha[U - 1] + (alpha[U - 2] if U > 1 else zero))


def test_spec_equals_autograd_of_a_direct_lattice():
  torch = pytest.importorskip('torch')
  rng = np.random.default_rng(2)
  shapes = [[W], [W, 0], [0, W], [1, W, 1], [W, 1, 1], [1, 1, W], [W, 0, W], [0, W, 1], [0, 0, W, 0], [W, 1, 0, W]]
  worst = [0.0, 0.0]
  for case in range(20):
    label = shapes[case % len(shapes)]
    C = (3, 4, 7, 31)[case % 4]
    label = [l if l == W else l % (C - 1) for l in label]
    T = WO.min_frames(label) + int(rng.integers(0, 4))
    bias = (-1.0, 0.0, -0.3, -4.0)[case % 4]
    x = rng.standard_normal((T, C)) * 2
    if case % 5 == 4:
      x[0, 0] = -np.inf                                         # (a dead class: the spec's -inf handling)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    ref = _torch_lattice_loss(xt, label, bias)
    ref.backward()
    loss, grad = WO.ctc_loss_and_grad(x, label, bias)
    worst = [max(worst[0], abs(loss - float(ref.detach()))), max(worst[1], float(np.max(np.abs(grad - xt.grad.numpy()))))]
  assert worst[0] < 1e-12 and worst[1] < 1e-12, worst


def test_spec_refusal_and_bias():
  x = AO.random_logits(np.random.default_rng(3), 3, 5)
  loss, grad = WO.ctc_loss_and_grad(x, [0, W, 0, 1], -1.0)              # four labels, three frames
  assert loss == np.inf and grad.shape == (3, 5) and not grad.any()
  l1, _ = WO.ctc_loss_and_grad(x, [0, W, 1], -1.0)                      # one path: every frame its state
  l0, _ = WO.ctc_loss_and_grad(x, [0, W, 1], 0.0)
  assert abs((l1 - l0) - 1.0) < 1e-12                                   # the wildcard's frame pays the bias


# ---- the case table -----------------------------------------------------------------------------------------------------------

def test_case_table_claims():
  assert WC.BATCH_NAMES == tuple(b.name for b in WC.all_batches())
  assert [b.k for b in WC.dispatch_batches()] == list(CC.KPLS) and {b.C for b in WC.dispatch_batches()} == {29}
  assert sorted((b.k, b.C) for b in WC.class_count_batches()) == [(k, C) for k in (1, 3) for C in (2, 3, 31)]
  ends = set()
  for b in WC.all_batches():
    ends.add(b.frames % 64)
    kinds = {u.kind: u for u in b.utterances}
    assert tuple(u.kind for u in b.utterances) == WC.KINDS
    assert CC.dispatch_of(max(len(u.label) for u in b.utterances)) == b.k                   # the dispatch this batch is for
    for u in b.utterances:
      assert u.logits.dtype == np.float32 and u.logits.shape == (u.logits.shape[0], b.C) and u.logits.shape[0] <= b.frames
      assert all(l == W or 0 <= l < b.C - 1 for l in u.label) and u.wild == (W in u.label)
      assert not any(p == W and q == W for p, q in zip(u.label, u.label[1:]))
      assert u.feasible == (WO.min_frames(u.label) <= u.logits.shape[0])
    # the longest label, wildcards on both boundary sets (and elsewhere)
    long = kinds['long']
    assert len(long.label) == CC.largest_label(b.k) and long.logits.shape[0] == b.frames
    crossing, last_slots = CC.boundary_indices(len(long.label), b.k)
    stars = {i for i, l in enumerate(long.label) if l == W}
    assert len(stars & set(crossing)) >= 2 and len(stars & set(last_slots)) >= 2 and 0 in stars
    neither = set(range(1, len(long.label))) - set(crossing) - set(last_slots)       # (empty for k <= 4: every index is on a boundary)
    assert not neither or stars & neither
    assert kinds['ends'].label[0] == W and kinds['ends'].label[-1] == W and kinds['ends'].logits.shape[0] % 64 in (63, 0, 1)
    assert kinds['w1'].label == [W] and kinds['w1'].logits.shape[0] == 1
    assert kinds['wedge'].label == [W] and kinds['wedge'].logits.shape[0] in CC.CHUNK_EDGES
    m = kinds['masked']
    dead = np.isneginf(m.logits[:, :b.C - 1]).all(axis=1)
    assert dead.sum() == 5 and np.isfinite(m.logits[:, b.C - 1]).all() and m.label.count(W) == 2
    assert not kinds['plain_a'].wild and not kinds['plain_b'].wild
    short = kinds['short']
    assert short.wild and WO.min_frames(short.label) == short.logits.shape[0] + 1 and not short.feasible
  assert ends == {63, 0, 1}


@pytest.mark.parametrize('name', ['wk1', 'wk2', 'wk1-C2', 'wk3-C31'])
def test_case_table_oracle_results(name):
  """Finite losses and gradients; the masked window gives the wildcard nothing (only the blank column moves there)."""
  batch = WC.batch_by_name(name)
  refs = WC.oracle_results(name)
  for u, ref in zip(batch.utterances, refs):
    if not u.feasible:
      assert ref is None
      continue
    loss, grad = ref
    assert np.isfinite(loss) and np.isfinite(grad).all() and grad.shape == u.logits.shape
    assert np.abs(grad.sum(axis=1)).max() < 1e-9                 # rows sum to zero: y sums to 1, the occupancies to 1
    if u.kind == 'masked':
      dead = np.isneginf(u.logits[:, :batch.C - 1]).all(axis=1)
      assert not grad[dead][:, :batch.C - 1].any()
    if u.kind == 'w1':
      # one frame, one path: loss = -ln w_0, the blank is pushed down by y(blank), the labels up in proportion to y(k) / S
      ly, log_s, _ = WO.emissions(u.logits, u.label, WC.BIAS)
      assert abs(loss + float(log_s[0] + WC.BIAS)) < 1e-12
      assert abs(grad[0, -1] - np.exp(ly[0, -1])) < 1e-12
      assert np.abs(grad[0, :-1] - (np.exp(ly[0, :-1]) - np.exp(ly[0, :-1] - log_s[0]))).max() < 1e-12


# ---- partial_labels -----------------------------------------------------------------------------------------------------------

def _ids(text):
  from speecht_amd import vocabulary
  return vocabulary.sentence_to_ids(text)


def test_partial_token_words():
  from speecht_amd import partial_labels as PL
  S = 27
  p = PL.PartialTranscripts()
  assert PL.WILDCARD == W == -1 and PL.WILDCARD_BIAS == -1.0 and _ids('*') == [-55]
  assert p.apply([_ids('a * b'), _ids('* a'), _ids('a *'), _ids('*'), _ids('ab'), []]) == \
      [[0, S, W, S, 1], [W, S, 0], [0, S, W], [W], [0, 1], []]
  assert p.apply([_ids('a * * b')]) == [[0, S, W, S, 1]]                # neighbouring wildcards are one
  for glued in ('a* b', 'a *b', 'a**b', '** a'):
    with pytest.raises(ValueError, match='outside|must lie'):
      p.apply([_ids(glued)])
  multi = PL.PartialTranscripts(token='<unk>')
  assert multi.apply([_ids('a <unk> b')]) == [[0, S, W, S, 1]]
  with pytest.raises(ValueError):
    multi.apply([_ids('a <unk b')])
  for bad in ('a', "it's", 'a b', ''):
    with pytest.raises(ValueError, match='outside the vocabulary'):
      PL.PartialTranscripts(token=bad)
  for kw in (dict(bias=0.5), dict(bias=float('nan')), dict(bias=float('-inf')), dict(drop=1.0), dict(drop=-0.1)):
    with pytest.raises(ValueError):
      PL.PartialTranscripts(**kw)


def test_partial_refuses_a_back_tick():
  """A back-tick is -1 under the reference's ord - 97 rule: it must not be read as the wildcard."""
  from speecht_amd import partial_labels as PL
  assert _ids('`') == [W]
  for p in (PL.PartialTranscripts(), PL.PartialTranscripts(ends=True), PL.PartialTranscripts(drop=0.5),
            PL.PartialTranscripts(token=None), PL.PartialTranscripts(token=None, ends=True), PL.PartialTranscripts(token=None, drop=0.5)):
    with pytest.raises(ValueError, match='must lie'):
      p.apply([_ids('a ` b')])
    with pytest.raises(ValueError):
      p.apply([_ids('a 1 b')])
    assert p.apply([_ids('a ` b'), _ids('a b')], defer=True)[0] == [PL.REFUSED]


def test_partial_without_a_token():
  """token=None: no word is read as a wildcard (a `*` is the id outside the vocabulary it always was), ends and drop still work."""
  from speecht_amd import partial_labels as PL
  S = 27
  assert PL.PartialTranscripts(token=None).apply([_ids('a b'), []]) == [[0, S, 1], []]
  assert PL.PartialTranscripts(token=None, ends=True).apply([_ids('a b')]) == [[W, S, 0, S, 1, S, W]]
  for text in ('a * b', '*', 'a ` b'):
    with pytest.raises(ValueError, match='must lie'):
      PL.PartialTranscripts(token=None, ends=True).apply([_ids(text)])
    assert PL.PartialTranscripts(token=None).apply([_ids(text)], defer=True) == [[PL.REFUSED]]


def test_partial_draw_ids_are_spec_augments():
  """partial_labels restates augmentation.draw_ids (that module binds the native library): the two must stay equal for the draws
  to follow the utterance as SpecAugment's do."""
  from speecht_amd import augmentation, partial_labels as PL
  for step, batch, world, rank in ((0, 1, 1, 0), (7, 4, 1, 0), (7, 4, 2, 1), (123456789, 32, 8, 5), (2 ** 40, 3, 4, 3)):
    a, b = augmentation.draw_ids(step, batch, world, rank), PL.draw_ids(step, batch, world, rank)
    assert a.dtype == b.dtype == np.int64 and np.array_equal(a, b)


def test_partial_ends():
  from speecht_amd import partial_labels as PL
  S = 27
  p = PL.PartialTranscripts(ends=True)
  assert p.apply([_ids('a b'), _ids('* a'), _ids('a *'), [], _ids('*')]) == \
      [[W, S, 0, S, 1, S, W], [W, S, 0, S, W], [W, S, 0, S, W], [W], [W]]


def test_partial_drop_is_a_function_of_seed_step_and_utterance():
  from speecht_amd import partial_labels as PL
  S = 27
  text = 'the quick brown fox jumps over the lazy dog and runs away'
  labels = [_ids(text)] * 8
  p = PL.PartialTranscripts(drop=0.4, seed=5)
  whole = p.apply(labels, step=7, rank=0, world=1)
  assert whole == p.apply(labels, step=7, rank=0, world=1)                                   # deterministic
  assert len({tuple(l) for l in whole}) > 4                                                   # per utterance
  # the same global utterance under two ranks of four, and under four ranks of two: the row of the batch does not matter
  assert whole == p.apply(labels[:4], 7, 0, 2) + p.apply(labels[4:], 7, 1, 2)
  assert whole == sum((p.apply(labels[2 * r:2 * r + 2], 7, r, 4) for r in range(4)), [])
  assert whole != p.apply(labels, step=8) and whole != PL.PartialTranscripts(drop=0.4, seed=6).apply(labels, step=7)
  words = text.split()
  for l in whole:
    assert not any(a == W and b == W for a, b in zip(l, l[1:]))
    kept = [w for w in ''.join('*' if i == W else 'abcdefghijklmnopqrstuvwxyz\' '[i] for i in l).split(' ')]
    assert '' not in kept and not any(a == '*' and b == '*' for a, b in zip(kept, kept[1:]))   # runs collapsed
    it = iter(words)
    assert all(w == '*' or w in it for w in kept)                                              # the kept words, in order
  # roughly the asked share of words goes
  many = p.apply([_ids(text)] * 200, step=1)
  share = 1 - np.mean([sum(w != '*' for w in ''.join('*' if i == W else 'x' if i != S else ' ' for i in l).split(' ')) for l in many]) / len(words)
  assert 0.3 < share < 0.5, share
  assert PL.PartialTranscripts(drop=0.0).apply(labels) == labels


def test_partial_drop_never_leaves_an_empty_transcript():
  from speecht_amd import partial_labels as PL
  p = PL.PartialTranscripts(drop=0.99, seed=1)
  for text in ('a', 'ab cd', 'a b c d e f'):
    out = p.apply([_ids(text)] * 50, step=3)
    assert all(any(i not in (W, 27) for i in l) for l in out)
    assert any(W in l for l in out) or text == 'a'
  assert p.apply([[], _ids('*')]) == [[], [W]]


def test_cli_flags():
  cli = _cli()
  from speecht_amd import partial_labels as PL
  _, flags = cli.parse(['train'])
  assert not any(hasattr(flags, f) for f in ('wildcard', 'wildcard_ends', 'wildcard_bias', 'wildcard_drop'))
  assert PL.from_flags(flags) is None
  _, flags = cli.parse(['train', '--wildcard'])
  p = PL.from_flags(flags)
  assert (p.token, p.ends, p.bias, p.drop) == ('*', False, -1.0, 0.0)
  _, flags = cli.parse(['train', '--wildcard', '<gap>', '--wildcard-ends', '--wildcard-bias', '-0.5', '--wildcard-drop', '0.2', '--seed', '9'])
  p = PL.from_flags(flags)
  assert (p.token, p.ends, p.bias, p.drop, p.seed) == ('<gap>', True, -0.5, 0.2, 9)
  _, flags = cli.parse(['train', '--wildcard-ends'])
  assert PL.from_flags(flags).ends and PL.from_flags(flags).token == '*'
  for bad in (['--wildcard-bias', '0.5'], ['--wildcard-bias', 'x'], ['--wildcard-drop', 'x'], ['--wildcard-drop', '1.0'],
              ['--wildcard-drop', '-0.1'], ['--wildcard-drop', 'nan']):
    with pytest.raises(SystemExit):
      cli.parse(['train'] + bad)
  with pytest.raises(SystemExit):
    cli.parse(['evaluate', '--wildcard'])


def test_header_lib_and_exports_agree():
  from speecht_amd import _lib
  lib = _lib.load()
  header = open(os.path.join(ROOT, 'include', 'speecht_hip.h')).read()
  name = 'st_ctc_loss_grad_wild_f32'
  assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS and 'int ' + name + '(' in header
  plain, wild = _lib._SIGNATURES['st_ctc_loss_grad_hilo_f32'], _lib._SIGNATURES[name]
  assert wild[0] is plain[0] and len(wild[1]) == len(plain[1]) + 1
  at = wild[1].index(ctypes.c_double)
  assert wild[1][:at] + wild[1][at + 1:] == plain[1] and plain[1][at - 1] is ctypes.c_float         # behind grad_scale
  decl = header[header.index('int ' + name + '('):]
  decl = decl[:decl.index(';')]
  assert 'float grad_scale, double wildcard_bias, float* loss' in ' '.join(decl.split())


def test_model_and_engine_take_the_option():
  import inspect
  pytest.importorskip('torch')
  from speecht_amd import engine, speech_model
  assert inspect.signature(engine.Wav2LetterEngine.set_labels).parameters['wildcard'].default is False
  assert inspect.signature(speech_model.SpeechModel.add_training_ops).parameters['partial'].default is None


# ---- the planted experiment (DESIGN.md "Training on partial transcripts") ---------------------------------------------------------

def test_planted_experiment():
  """Logits spell A X B -- 12 labels over 40 frames, 15 other labels over 50 frames, 12 over 40 -- and the transcript is A B.
  Plain CTC of `A B` has to explain X's frames with A's and B's labels and pushes the network there; wildcard CTC of `A * B` at
  bias -1.0 leaves them nearly alone.  Mean |g| on X's 50 frames, seed 2024: printed, and quoted in DESIGN.md."""
  rng = np.random.default_rng(2024)
  C = 29
  a, x, b = (AO.random_labels(rng, n, C, 0.1) for n in (12, 15, 12))
  parts = [AO.planted_logits(rng, lab, t, C, boost=8.0)[0] for lab, t in ((a, 40), (x, 50), (b, 40))]
  logits = np.concatenate(parts)
  _, g_plain = WO.ctc_loss_and_grad(logits, a + b)
  _, g_wild = WO.ctc_loss_and_grad(logits, a + [W] + b, -1.0)
  _, g_full = WO.ctc_loss_and_grad(logits, a + x + b)
  on_x = lambda g: float(np.mean(np.abs(g[40:90])))
  print('mean |g| on the left-out frames: plain CTC of A B {:.4g}, wildcard CTC of A * B {:.4g}, plain CTC of the full A X B {:.4g}'.format(
      on_x(g_plain), on_x(g_wild), on_x(g_full)))
  assert on_x(g_wild) < on_x(g_plain)
