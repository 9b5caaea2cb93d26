"""An engine's per-shape state at full width, where every production step runs in the frequency domain.

Real training changes (B, max_T) nearly every step.  A shape seen before is re-entered from a cached description
(Wav2LetterEngine._reenter_shape: the cached ShapeState object made `engine.shape` again, the logged byte ranges
re-zeroed, freshness re-evaluated by the mode); a tuning knob flipped on a live engine makes it describe the shape anew and
rebuild every operand derived from the weights.  Either way every step must equal, bit for bit, the same step on an engine
built fresh from the same params, m, v and step count.  The walks use the model's own widths (250 / 2000 channels, non-zero
biases) and assert from the launch trace that they cross each boundary of the regime they are meant to cover.
"""
import gc
import re

import numpy as np
import pytest

from tests import workloads as WL

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


# B * T' after the stride-2 first layer (T' = ceil(T / 2)); blocks of 64 frames per utterance in the frequency domain
SHAPES = {
    'D': [201] * 30 + [150, 101],       # 3 232 rows, 2 blocks, 64 rows per bin: every layer spectral, fused transforms
    'F': [401, 333],                    # 402 rows: W-tap kernels everywhere, reductions split over the idle CUs
    'E': [601] * 18 + [555, 480],       # 6 020 rows, 5 blocks, 100 rows per bin (not a multiple of 64): separate transforms
    'B': [1533] * 6 + [1400, 1100],     # short batch of long utterances: 12 blocks, 96 rows per bin (stream-K products)
    'G': [801] * 3 + [700],             # 1 604 rows: the 32-tap layer spectral, the 7-tap layers and the first layer not
    'H': [400] * 2 + [390],             # 600 rows, even max_T: W-tap everywhere
    'J': [301] * 62 + [280, 250],       # 9 664 rows, 3 blocks, 192 rows per bin: a last half tile of 64 rows
    'I': [1000] * 16,                   # 8 000 rows, even max_T, 8 blocks, 128 rows per bin: fused transforms
}
# ten of the eighteen steps re-enter a cached shape; consecutive steps cross the boundaries each walk lists (`run_walk`)
WALK = ['D', 'F', 'E', 'D', 'B', 'F', 'G', 'E', 'H', 'G', 'J', 'B', 'D', 'H', 'I', 'E', 'I', 'F']


def make_engine(layers, dev, mode):
  from speecht_amd.engine import Wav2LetterEngine
  return Wav2LetterEngine(layers, device=dev, conv_mode=mode)


def one_step(e, frames, mel, seed):
  x, seq, labels = WL.make_batch(frames, mel, seed=seed)
  e.load_batch(x, seq)
  e.set_labels(labels)
  e.forward()
  e.ctc_loss_grad(1.0 / len(frames))
  e.backward()
  logits, grads, loss = e.X[-1].interior().clone(), e.grads.clone(), e.loss.clone()
  e.apply_update(1e-3)
  torch.cuda.synchronize()
  return logits, grads, loss, e.params.clone(), e.adam_m.clone(), e.adam_v.clone()


def fresh_like(eng, layers, dev, mode):
  fresh = make_engine(layers, dev, mode)
  for name in ('params', 'adam_m', 'adam_v'):
    getattr(fresh, name).copy_(getattr(eng, name))
  fresh.step_count = eng.step_count
  fresh.mark_weights_changed()
  return fresh


def assert_same(a, b, where):
  for what, u, v in zip(('logits', 'gradients', 'losses', 'weights', 'm', 'v'), a, b):
    assert torch.equal(u, v), (where, what, float((u - v).abs().max()))


def features(lines):
  """What the trace of one training step says about the regime it ran in."""
  rows = [int(m.group(1)) for l in lines if ' batched ' in l for m in [re.search(r' M=(\d+)', l)] if m]
  wtap = [l for l in lines if l.startswith(('gemm_nn<', 'gemm_nn_bf16<', 'conv_taps_bf16<'))]      # (filters_idft_* name taps too)
  splits = [int(m.group(1)) for l in wtap if ' taps=7 ' in l for m in [re.search(r' splits=(\d+)', l)] if m]
  return {
      'W-tap 7-tap layers': any(' taps=7 ' in l for l in wtap),
      'W-tap 32-tap layer': any(' taps=32 ' in l for l in wtap),
      'fused transforms': any(l.startswith('idft_dft_rows') for l in lines),
      'stream-K products': any(' streamk ' in l for l in lines),
      'half-tile launch': any(m % 128 == 64 and m > 128 for m in rows),
      'split W-tap reductions': any(s > 1 for s in splits),
  }


def run_walk(dev, mode, mel, expect):
  from speecht_amd._lib import launch_trace
  layers = WL.w2l_layers(mel)
  params = WL.xavier_params(layers, seed=42, dtype=np.float32)      # non-zero biases
  eng = make_engine(layers, dev, mode)
  eng.set_weights(params)
  # buffers at the size of the largest shape first (what `reserve` does for a ladder of lengths): a buffer that grows starts a new
  # storage generation and drops every cached description with it; then the cache starts empty, so that first visits describe
  for _ in range(2):
    for frames in SHAPES.values():
      eng._ensure_shape(len(frames), max(frames))
  eng._shape_cache.clear()
  generation = eng._storage.generation
  reentered, seen = 0, []
  for k, name in enumerate(WALK):
    frames = SHAPES[name]
    shape = (len(frames), max(frames))
    reentered += int(shape in (eng.__dict__.get('_shape_cache') or {}) and eng._shape != shape)
    fresh = fresh_like(eng, layers, dev, mode)
    with launch_trace() as tr:
      a = one_step(eng, frames, mel, 500 + k)
    b = one_step(fresh, frames, mel, 500 + k)
    assert_same(a, b, (mode, mel, k, name))
    f = features(tr.lines)
    f['first layer spectral'] = 0 in eng.fft
    f['7-tap layers spectral'] = 1 in eng.fft
    f['32-tap layer spectral'] = 8 in (eng.fft if mode != 'bf16' else eng.fftb)
    f['odd max_T'] = shape[1] % 2 == 1
    seen.append((name, f, tr.lines))
    del fresh, a, b
    gc.collect()
  for name, f, lines in seen:         # (the record a reader of `pytest -s` sees: regime per step)
    print(mode, mel, name, sorted(k for k, v in f.items() if v))
  assert reentered >= len(WALK) // 2, reentered
  assert eng._storage.generation == generation
  # the walk crosses every boundary it is meant to: some pair of consecutive steps differs in it
  for key in expect:
    assert any(s[1][key] != t[1][key] for s, t in zip(seen, seen[1:])), (key, [(n, f[key]) for n, f, _ in seen])
  return eng, seen


def test_full_width_walk_fp32_80_mel(dev):
  eng, seen = run_walk(dev, 'fp32', 80, ['first layer spectral', '7-tap layers spectral', '32-tap layer spectral', 'W-tap 7-tap layers',
                                         'W-tap 32-tap layer', 'fused transforms', 'stream-K products', 'half-tile launch',
                                         'split W-tap reductions', 'odd max_T'])
  for name, f, lines in seen:
    # the trace agrees with the engine's own choice of layers
    assert f['W-tap 7-tap layers'] == (not f['7-tap layers spectral']), (name, f)
    assert f['W-tap 32-tap layer'] == (not f['32-tap layer spectral']), (name, f)
    assert f['first layer spectral'] == f['7-tap layers spectral'], (name, f)          # one threshold, 3 000 rows


def test_full_width_walk_fp32_128_mel(dev):
  eng, seen = run_walk(dev, 'fp32', 128, ['first layer spectral', '32-tap layer spectral', 'fused transforms', 'odd max_T'])
  # 128 mel: the polyphase first layer reads 2 x 128 channels, whose spectra halves tile the split lag products
  assert any(f['first layer spectral'] for _, f, _ in seen)


def test_full_width_walk_bf16(dev):
  # bf16 activations: the 32-tap layer's plane path joins and leaves the set at 1 000 rows
  eng, seen = run_walk(dev, 'bf16', 80, ['32-tap layer spectral', 'W-tap 32-tap layer', 'odd max_T'])
  for name, f, lines in seen:
    assert f['W-tap 32-tap layer'] == (not f['32-tap layer spectral']), (name, f)


# ---- per-shape state lives in ONE object ---------------------------------------------------------------------------------

# what a description may change on the engine and on the mode: the current ShapeState, the cache, and the mode's cross-shape
# state that a transition between shapes recomputes on purpose
RECOMPUTED = {
    'shape',               # the current ShapeState (everything that is a function of the shape is inside it)
    '_shape_cache',        # the cache (a new entry)
    '_fft_prev', '_fftb_prev',                                 # the frequency-domain set left behind: `_fft_transition` compares
    '_fft_table_key', '_fftb_table_key',                       # whose tables lie in each layer's buffer: checked against the state's keys
    '_gfwd_fresh', '_packed_t_fresh', '_wplanes_fresh', '_wtplanes_fresh',   # freshness flags, re-evaluated by the transitions
}


def snapshot(d):
  def shallow(v):
    if isinstance(v, dict):
      return tuple((k, id(x)) for k, x in v.items())
    if isinstance(v, (list, tuple, set, frozenset)):
      return tuple(sorted(id(x) for x in v))
    return None
  return {k: (v, shallow(v)) for k, v in d.items()}


def changed(before, after):
  out = {k for k, (v, shallow) in after.items() if k not in before or before[k][0] is not v or before[k][1] != shallow}
  return out | (set(before) - set(after))


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
def test_every_per_shape_attribute_is_cached_or_recomputed(dev, mode):
  """Describe two shapes on the frequency-domain path on one engine: the only engine or mode attributes the second description
  changed are `shape`, the cache and what a transition recomputes on purpose (RECOMPUTED) -- a per-shape value kept anywhere
  but in the ShapeState fails this.  Going back to the first shape makes the very object described first current again."""
  layers = WL.w2l_layers(80)
  eng = make_engine(layers, dev, mode)
  eng.set_weights(WL.xavier_params(layers, seed=42, dtype=np.float32))
  # (buffers at their final size first, as in `run_walk`: a buffer that grows drops every cached description)
  for _ in range(2):
    for name in ('D', 'E'):
      eng._ensure_shape(len(SHAPES[name]), max(SHAPES[name]))
  eng._shape_cache.clear()
  generation = eng._storage.generation
  eng._ensure_shape(len(SHAPES['D']), max(SHAPES['D']))
  assert 8 in (eng.fft if mode != 'bf16' else eng.fftb)
  first, first_x0, first_part = eng.shape, eng.shape.X[0].buf.data_ptr(), eng.shape.mode
  before, mode_before = snapshot(eng.__dict__), snapshot(eng.mode.__dict__)
  eng._ensure_shape(len(SHAPES['E']), max(SHAPES['E']))
  assert 8 in (eng.fft if mode != 'bf16' else eng.fftb)
  allowed = RECOMPUTED
  diff = changed(before, snapshot(eng.__dict__)) | changed(mode_before, snapshot(eng.mode.__dict__))
  assert diff, 'nothing changed between two shapes: the snapshot is broken'
  assert diff <= allowed, sorted(diff - allowed)
  assert eng.shape is not first
  eng._ensure_shape(len(SHAPES['D']), max(SHAPES['D']))
  assert eng.shape is first and eng._storage.generation == generation
  assert eng.shape.X[0].buf.data_ptr() == first_x0 and eng.shape.mode is first_part


# ---- knobs flipped on a live engine ----------------------------------------------------------------------------------------

# knob, value, mode, shape: one where the knob's kernel is on the path (streamk_test_drop is a fault-injection hook: not here;
# no_g3 changes nothing on the bf16 path, whose 32-tap layer runs its products on one bf16 plane)
KNOBS = [
    ('streamk', 1, 'fp32', 'D'), ('streamk', 2, 'fp32', 'B'), ('streamk_slots', 96, 'fp32', 'B'),
    ('no_fused_transforms', 1, 'fp32', 'D'), ('filters_idft_valu', 1, 'fp32', 'D'), ('no_g3', 1, 'fp32', 'D'),
    ('g3_tile', 1, 'fp32', 'D'), ('g3_tile', 2, 'fp32', 'D'), ('g3_tile', 4, 'fp32', 'D'),
    ('bf16_lag_copies', 1, 'bf16', 'D'), ('bf16_taps_panel', 1, 'bf16', 'I'),
]


@pytest.mark.parametrize('knob,value,mode,shape', KNOBS, ids=['{}={}-{}'.format(k, v, m) for k, v, m, _ in KNOBS])
def test_knob_flipped_on_a_live_engine(dev, knob, value, mode, shape):
  """One step, the knob flipped, the same batch again, the knob back, the batch again: every step after a flip equals, bit for bit,
  the step of a fresh engine built under the same setting, and the trace shows that the knob changed what ran."""
  from speecht_amd._lib import launch_trace, set_tuning
  layers = WL.w2l_layers(80)
  frames = SHAPES[shape]
  eng = make_engine(layers, dev, mode)
  eng.set_weights(WL.xavier_params(layers, seed=42, dtype=np.float32))
  traces = []
  try:
    for setting in (0, value, 0):
      set_tuning(knob, setting)
      fresh = fresh_like(eng, layers, dev, mode)
      with launch_trace() as tr:
        a = one_step(eng, frames, 80, 700)
      b = one_step(fresh, frames, 80, 700)
      assert_same(a, b, (knob, setting))
      traces.append(sorted(re.sub(r' (gflop|mb)=\S+', '', l) for l in tr.lines))
      del fresh, a, b
      gc.collect()
  finally:
    set_tuning(knob, 0)
  print(knob, value, mode, 'only with the knob:', sorted(set(traces[1]) - set(traces[0]))[:2], 'only without:',
        sorted(set(traces[0]) - set(traces[1]))[:2])
  assert traces[1] != traces[0], (knob, 'the knob changed nothing at this shape')
