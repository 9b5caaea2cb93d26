"""What a training step leaves behind for the next one: clip + Adam at the edges of its kernel, and skipped updates.

clip_adam_kernel (csrc/optim.hip) skips the update when CTC rejected the batch (the gate) or when the global gradient norm is not
finite.  A skipped update must leave params, m and v as they were, bit for bit, and must not count: every applied update uses
t = 1 + the number of updates applied before it, and the engine's step count, SpeechModel.global_step and the beta powers of a
TF checkpoint all count applied updates only.  Applied updates are held against float64 (oracle.w2l_oracle) at the tolerances of
test_gpu_parity.test_clip_adam.
"""
import ctypes
import math
import warnings

import numpy as np
import pytest

from oracle import w2l_oracle as O
from tests import workloads as WL

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

# clip_adam_kernel runs at most 2048 workgroups of 256 threads over 4-float vectors: the first size whose vectors reach the
# grid-stride loop (a second pass of workgroup 0), with a ragged tail of one element behind them
GRID_STRIDE_N = 2048 * 256 * 4 + 13
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-3


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def host_rate(t, lr=LR):
  return lr * math.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t)


def run_update(dev, entry, p, g, m, v, clip, step=3, gate=0.0, applied=None):
  """One call of a clip + Adam entry point on float32 copies of p, g, m, v.  ``entry``: 'gated' (lr_t from the host) or 'counted'
  (the device count of applied updates: ``applied``, default step - 1).  Returns the device buffers, stats, counts (or None)."""
  from speecht_amd import _lib
  t = [torch.as_tensor(np.asarray(a, dtype=np.float32)).to(dev) for a in (p, g, m, v)]
  stats = torch.full((4,), -1.0, device=dev)
  gate_t = torch.tensor([gate, 0.0], dtype=torch.float32, device=dev)
  ws = torch.zeros(_lib.load().st_global_norm_ws(len(p)) // 4, device=dev)
  P = lambda x: ctypes.c_void_p(x.data_ptr())
  counts = None
  if entry == 'gated':
    _lib.call('st_global_norm_clip_adam_gated_f32', P(t[0]), P(t[1]), P(t[2]), P(t[3]), len(p), clip, float(host_rate(step)), B1, B2,
              EPS, P(stats), P(gate_t), P(ws), ws.numel() * 4, None)
  else:
    counts = torch.tensor([step - 1 if applied is None else applied, 7], dtype=torch.int32, device=dev)
    _lib.call('st_global_norm_clip_adam_counted_f32', P(t[0]), P(t[1]), P(t[2]), P(t[3]), len(p), clip, LR, B1, B2, EPS, P(stats),
              P(gate_t), P(counts), P(ws), ws.numel() * 4, None)
  torch.cuda.synchronize()
  return [x.cpu().numpy() for x in t], stats.cpu().numpy(), (None if counts is None else counts.cpu().numpy())


def inputs(n, seed, gscale=1.0):
  rng = np.random.default_rng(seed)
  p = rng.standard_normal(n).astype(np.float32)
  g = (rng.standard_normal(n) * gscale).astype(np.float32)
  m = (rng.standard_normal(n) * 0.1).astype(np.float32)
  v = (rng.random(n) * 0.01).astype(np.float32)
  return p, g, m, v


def assert_applied(out, stats, p, g, m, v, clip, step):
  g64, p64, m64, v64 = (a.astype(np.float64) for a in (g, p, m, v))
  clipped, gn = O.clip_by_global_norm([g64], clip)
  pr, mr, vr = O.adam_tf_step(p64, clipped[0], m64, v64, step, LR)
  assert float(stats[0]) == pytest.approx(gn, rel=1e-5)
  assert float(stats[1]) == pytest.approx(clip / max(gn, clip), rel=1e-5)
  np.testing.assert_allclose(out[0], pr, rtol=2e-5, atol=1e-6)
  np.testing.assert_allclose(out[2], mr, rtol=2e-5, atol=1e-7)
  np.testing.assert_allclose(out[3], vr, rtol=2e-5, atol=1e-9)


def assert_untouched(out, p, m, v):
  for got, want in ((out[0], p), (out[2], m), (out[3], v)):
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize('entry', ['gated', 'counted'])
@pytest.mark.parametrize('n', [1, 3, 5, 4099, GRID_STRIDE_N])
def test_clip_adam_sizes_against_float64(dev, entry, n):
  """Below one vector, one vector + tail, many workgroups, and the grid-stride loop with a ragged tail; clipped (norm >> 5)."""
  p, g, m, v = inputs(n, seed=n, gscale=3.0)
  out, stats, counts = run_update(dev, entry, p, g, m, v, clip=5.0 if n > 5 else 0.5)
  assert_applied(out, stats, p, g, m, v, 5.0 if n > 5 else 0.5, 3)
  if counts is not None:
    assert counts.tolist() == [3, 7]                     # applied: counted; the skip count untouched
    assert stats[2] == np.float32(host_rate(3))


def poison_positions(n):
  pos = {'first vector': 1}
  if n >= GRID_STRIDE_N:
    pos['grid-stride part'] = 2048 * 256 * 4 + 2
  if n % 4:
    pos['tail'] = n - 1
  return pos


@pytest.mark.parametrize('entry', ['gated', 'counted'])
@pytest.mark.parametrize('n', [5, 4099, GRID_STRIDE_N])
def test_one_non_finite_gradient_skips_the_update(dev, entry, n):
  """One NaN, +Inf or -Inf among finite gradients, in the first vector, in the grid-stride part and in the n % 4 tail: params,
  m and v unchanged bit for bit, stats[0] not finite, and (counted form) the applied count stays while the skip count moves."""
  base = inputs(n, seed=100 + n)
  for where, k in poison_positions(n).items():
    for bad in (np.nan, np.inf, -np.inf):
      p, g, m, v = (a.copy() for a in base)
      g[k] = bad
      out, stats, counts = run_update(dev, entry, p, g, m, v, clip=5.0)
      assert_untouched(out, p, m, v)
      assert not np.isfinite(stats[0]), (where, bad, stats)
      if counts is not None:
        assert counts.tolist() == [2, 8], (where, bad, counts)


@pytest.mark.parametrize('entry', ['gated', 'counted'])
def test_finite_gradients_whose_squares_overflow_skip_the_update(dev, entry):
  """|g| ~ 1e20: every gradient is finite, their sum of squares is not (fp32): the norm is +Inf and the update is skipped (the
  reference's tf.clip_by_global_norm would turn every gradient into NaN there)."""
  p, g, m, v = inputs(4099, seed=7)
  g = (np.sign(g) * 1e20).astype(np.float32)
  out, stats, counts = run_update(dev, entry, p, g, m, v, clip=5.0)
  assert np.isfinite(g).all()
  assert_untouched(out, p, m, v)
  assert stats[0] == np.inf
  if counts is not None:
    assert counts.tolist() == [2, 8]


@pytest.mark.parametrize('entry', ['gated', 'counted'])
@pytest.mark.parametrize('n', [3, GRID_STRIDE_N])
def test_gate_skips_a_finite_update_and_reports_the_norm(dev, entry, n):
  p, g, m, v = inputs(n, seed=300 + n)
  out, stats, counts = run_update(dev, entry, p, g, m, v, clip=5.0, gate=2.0)
  assert_untouched(out, p, m, v)
  gn = math.sqrt(float(np.sum(g.astype(np.float64) ** 2)))
  assert float(stats[0]) == pytest.approx(gn, rel=1e-5)
  if counts is not None:
    assert counts.tolist() == [2, 7]                     # a gated update is neither applied nor a non-finite skip


@pytest.mark.parametrize('entry', ['gated', 'counted'])
def test_norm_exactly_at_clip(dev, entry):
  """||g|| == clip exactly (3-4-5 in fp32): scale 1, the gradients pass unscaled."""
  n = 4099
  p, _, m, v = inputs(n, seed=11)
  g = np.zeros(n, np.float32)
  g[0], g[n - 1] = 3.0, 4.0
  out, stats, counts = run_update(dev, entry, p, g, m, v, clip=5.0)
  assert stats[0] == np.float32(5.0) and stats[1] == np.float32(1.0)
  assert_applied(out, stats, p, g, m, v, 5.0, 3)


@pytest.mark.parametrize('n', [4099, GRID_STRIDE_N])
def test_counted_update_writes_the_bits_of_the_host_rate_form(dev, n):
  """Same inputs, same t: the counted form (rate from the device count) and the gated form (rate from the host) write identical
  params, m and v -- the device count changes where t comes from, not the arithmetic of the update."""
  p, g, m, v = inputs(n, seed=900 + n, gscale=0.5)
  for step in (1, 2, 37):
    a, sa, _ = run_update(dev, 'gated', p, g, m, v, clip=5.0, step=step)
    b, sb, _ = run_update(dev, 'counted', p, g, m, v, clip=5.0, step=step)
    for x, y in zip(a, b):
      assert x.tobytes() == y.tobytes(), step
    assert sa[:2].tobytes() == sb[:2].tobytes()


def test_counted_rate_matches_the_host_formula(dev):
  """The counted form derives lr_t from the device count in double: the same float32 as the host formula it replaces, and the
  update of that t against float64."""
  n = 1000
  p, g, m, v = inputs(n, seed=5, gscale=0.01)
  for applied in (0, 1, 2, 9, 99, 999, 12345, 10 ** 6, 2 ** 31 - 2):
    out, stats, counts = run_update(dev, 'counted', p, g, m, v, clip=5.0, applied=applied)
    assert stats[2] == np.float32(host_rate(applied + 1)), (applied, stats[2], host_rate(applied + 1))
    assert counts.tolist() == [applied + 1, 7]
    assert_applied(out, stats, p, g, m, v, 5.0, applied + 1)


# ---- the engine --------------------------------------------------------------------------------------------------------------

def small_engine(dev, mode):
  from speecht_amd.engine import Wav2LetterEngine
  return Wav2LetterEngine(WL.w2l_layers(16, width=40, fc=72), device=dev, conv_mode=mode)


def backward_step(e, k):
  x, seq, labels = WL.make_batch([97, 80, 61], 16, seed=40 + k)
  e.load_batch(x, seq)
  e.set_labels(labels)
  e.forward()
  e.ctc_loss_grad(1.0 / 3)
  e.backward()


@pytest.mark.parametrize('mode', ['fp32', 'bf16', 'bf16x6'])
def test_poisoned_gradient_leaves_the_engine_state_and_the_next_step_is_exact(dev, mode):
  """NaN, then Inf, written into the flat gradients between backward() and apply_update(): params, m, v unchanged bit for bit,
  the step count unchanged and the skip visible; the next good step equals, bit for bit, the same step on a fresh engine given
  the same params, m, v and applied-update count."""
  eng = small_engine(dev, mode)
  eng.set_weights(WL.xavier_params(WL.w2l_layers(16, width=40, fc=72), seed=3))
  backward_step(eng, 0)
  eng.apply_update(LR)
  assert eng.step_count == 1 and eng.updates_skipped == 0
  k = 0
  for bad in (float('nan'), float('inf')):
    k += 1
    backward_step(eng, k)
    snap = [t.clone() for t in (eng.params, eng.adam_m, eng.adam_v)]
    eng.grads[eng.n_flat // 2 + 1] = bad
    eng.apply_update(LR)
    torch.cuda.synchronize()
    for a, b in zip(snap, (eng.params, eng.adam_m, eng.adam_v)):
      assert torch.equal(a, b), (mode, bad)
    assert eng.step_count == 1 and eng.updates_skipped == k, (eng.step_count, eng.updates_skipped)
    assert not math.isfinite(eng.last_skip_norm) and not math.isfinite(float(eng.stats[0]))
    # the next good step, here and on a fresh engine built from the same state
    fresh = small_engine(dev, mode)
    for name in ('params', 'adam_m', 'adam_v'):
      getattr(fresh, name).copy_(getattr(eng, name))
    fresh.step_count = eng.step_count
    fresh.mark_weights_changed()
    outs = []
    for e in (eng, fresh):
      backward_step(e, 10 + k)
      grads = e.grads.clone()
      e.apply_update(LR)
      torch.cuda.synchronize()
      outs.append((e.X[-1].interior().clone(), e.loss.clone(), grads, e.params.clone(), e.adam_m.clone(), e.adam_v.clone(),
                   e.stats[2].clone()))
    for what, a, b in zip(('logits', 'losses', 'gradients', 'weights', 'm', 'v', 'lr_t'), *outs):
      assert torch.equal(a, b), (mode, bad, what)
    assert float(outs[0][-1]) == np.float32(host_rate(2))              # t = 2: the skipped update did not count
    assert eng.step_count == 2 and fresh.step_count == 2
    del fresh
    # back to one applied update for the next poison (the counts are the engine's state, settable like the weights)
    eng.params.copy_(snap[0]); eng.adam_m.copy_(snap[1]); eng.adam_v.copy_(snap[2])
    eng.step_count = 1
    eng.mark_weights_changed()


def test_model_counts_applied_updates_only(dev, tmp_path):
  """Through SpeechModel.step: a poisoned step is skipped on the device; the next step's read-back reports it, global_step is
  taken back with a warning that names the step, and global_step, the engine's step count and the beta powers save_tf writes
  count applied updates only -- also when the checkpoint is written right behind the poisoned step."""
  from speecht_amd import tf_checkpoint as tfc
  from speecht_amd.speech_input import Coordinator, InputBatchLoader
  from speecht_amd.speech_model import Session, create_default_model

  class Flags:
    command = 'train'
    learning_rate = 1e-3
    learning_rate_decay_factor = 0
    max_gradient_norm = 5.0
    momentum = 0.9
    log_dir = str(tmp_path / 'log')
    run_name = 'unit'
    run_type = 'train'

  x, seq, labels = WL.make_batch([60, 60, 44, 60], 16, seed=5)

  def gen():
    while True:
      for i in range(4):
        yield x[i, :seq[i]], labels[i]
  loader = InputBatchLoader(16, 4, gen)
  coord = Coordinator()
  loader.start_threads(None, coord)
  model = create_default_model(Flags(), 16, loader)
  try:
    with Session(dev) as sess:
      model.init_session(sess)
      eng = model.engine
      update = eng.apply_update
      poison = []

      def apply_update(*a, **k):
        if poison:
          eng.grads[poison.pop()] = float('nan')
        return update(*a, **k)
      eng.apply_update = apply_update

      model.step(sess)                                      # applied: 1
      poison.append(12345)
      snap = [t.clone() for t in (eng.params, eng.adam_m, eng.adam_v)]
      with warnings.catch_warnings():
        warnings.simplefilter('error')
        model.step(sess)                                    # skipped on the device; the host does not know yet
      torch.cuda.synchronize()
      assert all(torch.equal(a, b) for a, b in zip(snap, (eng.params, eng.adam_m, eng.adam_v)))
      with pytest.warns(RuntimeWarning, match='update of training step 2 skipped'):
        model.step(sess)                                    # its read-back reports the skip; this step's update is applied
      assert model.global_step.eval() == 2 and eng.step_count == 2 and eng.updates_skipped == 1
      # a checkpoint right behind a poisoned step: the save waits for it and counts it out
      poison.append(7)
      model.step(sess)
      with pytest.warns(RuntimeWarning, match='update of training step 3 skipped'):
        prefix = model.saver.save_tf(sess, str(tmp_path / 'speechT.ckpt'), global_step=model.global_step)
      assert model.global_step.eval() == 2 and eng.step_count == 2 and eng.updates_skipped == 2
      saved = tfc.read_bundle(prefix)
      assert int(saved['Variable']) == 2
      assert saved['training/beta1_power'] == np.float32(0.9 ** 3)
      assert saved['training/beta2_power'] == np.float32(0.999 ** 3)
      model.step(sess)
      assert model.global_step.eval() == 3 and eng.step_count == 3 and eng.updates_skipped == 2
  finally:
    coord.request_stop()
