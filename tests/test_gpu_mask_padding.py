"""Masked batches: `engine.forward(mask_padding=True)` zeroes every utterance's rows past its own length after every layer but the
last, so a batched utterance gets the logits it gets alone (SAME padding puts the same zeros there).

Bounds.  Masked against solo is the same product in two summation orders (a batch of another size takes other tiles and splits):
1e-5 x max(1, max |logits|), the bound tests/test_gpu_parity.py uses for that (split against unsplit reduction).  Against the
float64 oracle on the unpadded input: 1e-5 absolute, the bound of tests/test_gpu_parity.py's small-stack logits check."""
import numpy as np
import pytest

from oracle import w2l_oracle as O
from tests import workloads as WL

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

SMALL_LAYERS = [(48, 2, 16, 32, True), (7, 1, 32, 32, True), (32, 1, 32, 40, True), (1, 1, 40, 29, False)]
SMALL_LENS = [57, 120, 121]
TAIL = 73                      # output frames before an utterance's end that see the padding (receptive field of the stack)


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def batch_of(lens, width, seed, frames=None):
  x = np.zeros((len(lens), frames or max(lens), width))
  for b, n in enumerate(lens):
    x[b, :n] = WL.synthetic_features(seed + b, n, width)
  return x


def logits_of(eng):
  torch.cuda.synchronize()
  return eng.X[-1].interior().cpu().numpy().astype(np.float64)          # [B, T', C]


def solo_runs(eng, x, lens, decode=False):
  """Every utterance alone, B = 1 and T = its own length: -> list of [ceil(len / 2), C] logits (and the greedy ids)."""
  out, ids = [], []
  for b, n in enumerate(lens):
    eng.load_batch(x[b:b + 1, :n], [n])
    eng.forward()
    if decode:
      ids.append(eng.greedy_decode()[0][0])
    out.append(logits_of(eng)[0])
    assert out[-1].shape[0] == -(-n // 2)
  return (out, ids) if decode else out


@pytest.fixture(scope='module')
def small(dev):
  from speecht_amd.engine import Wav2LetterEngine
  params = WL.xavier_params(SMALL_LAYERS, seed=21)                       # (biases in +-0.05: padding rows are not zero unmasked)
  x = batch_of(SMALL_LENS, 16, seed=40)
  ref = [np.transpose(O.wav2letter_forward(x[b:b + 1, :n], params, SMALL_LAYERS), (1, 0, 2))[0] for b, n in enumerate(SMALL_LENS)]
  def engine(mode):
    eng = Wav2LetterEngine(SMALL_LAYERS, device=dev, conv_mode=mode)
    eng.set_weights(params)
    return eng
  return dict(params=params, x=x, ref=ref, engine=engine)


def test_small_stack_masked_equals_solo(small):
  eng, x, lens = small['engine']('fp32'), small['x'], SMALL_LENS
  solo = solo_runs(eng, x, lens)
  eng.load_batch(x, lens)
  eng.forward(mask_padding=True)
  masked = logits_of(eng)
  for b, n in enumerate(lens):
    v = -(-n // 2)
    bound = 1e-5 * max(1.0, float(np.max(np.abs(solo[b]))))
    err, err64 = float(np.max(np.abs(masked[b, :v] - solo[b]))), float(np.max(np.abs(masked[b, :v] - small['ref'][b])))
    print('len {}: max |masked - solo| = {:.3e} (bound {:.1e}), max |masked - float64| = {:.3e}'.format(n, err, bound, err64))
    assert err < bound
    assert err64 < 1e-5
  # every intermediate row past the valid length is exactly zero, halo rows included
  for i in range(1, len(SMALL_LAYERS)):
    t = eng.X[i]
    full = t.buf.view(t.batch, t.t_pitch, t.c_pitch).cpu().numpy()
    for b, n in enumerate(lens):
      v = -(-n // 2)
      assert not full[b, t.halo + v:].any(), (i, b)
      assert not full[b, :t.halo].any(), (i, b)
      assert full[b, t.halo:t.halo + v, :t.channels].any(), (i, b)
  # unmasked, the last frames of the shorter utterances see the batch's padding: the test can tell the difference
  eng.forward()
  plain = logits_of(eng)
  worst = 0.0
  for b, n in enumerate(lens):
    v = -(-n // 2)
    if n < max(lens):
      d = float(np.max(np.abs(plain[b, max(0, v - TAIL):v] - solo[b][max(0, v - TAIL):])))
      print('len {}: unmasked, max |batched - solo| over the last {} frames = {:.3e}'.format(n, TAIL, d))
      worst = max(worst, d / max(1.0, float(np.max(np.abs(solo[b])))))
  assert worst > 1e-5
  # ... and masking again after an unmasked pass gives the masked logits again (nothing is left behind by either)
  eng.forward(mask_padding=True)
  assert np.array_equal(logits_of(eng), masked)


def test_full_model_masked_on_the_frequency_domain_chain(dev):
  """The eleven-layer model at B = 8, 128 mel bands, utterances of 500 to 800 frames in a batch padded to T = 1000: 500 output
  frames are 8 blocks of 64 per utterance, 64 rows per bin with no pad rows, which is what the hand-off needs (T = 800 gives 7
  blocks, 56 rows padded to 64, and the separate transforms).  Unmasked, the frequency-domain layers hand their spectra on
  (idft_dft_rows launches); masked, none does and ten st_mask_rows launches run; masked rows equal the solo runs and decode to
  the same ids -- the longest utterance's too, which here has padding of its own."""
  from speecht_amd._lib import launch_trace
  from speecht_amd.engine import Wav2LetterEngine
  layers = WL.w2l_layers(128)
  params = WL.xavier_params(layers, seed=33)
  lens = [500, 537, 601, 644, 699, 750, 777, 800]
  x = batch_of(lens, 128, seed=60, frames=1000)
  eng = Wav2LetterEngine(layers, device=dev, conv_mode='fp32')
  eng.set_weights(params)
  solo, solo_ids = solo_runs(eng, x, lens, decode=True)
  eng.load_batch(x, lens)
  with launch_trace() as tr:
    eng.forward()
  torch.cuda.synchronize()
  text = '\n'.join(tr.lines)
  assert sum(1 for l in tr.lines if l.startswith('idft_dft_rows<')) > 0, text            # the chain with hand-off
  assert not any(l.startswith('mask_rows') for l in tr.lines), text
  with launch_trace() as tr:
    eng.forward(mask_padding=True)
  ids = eng.greedy_decode()[0]
  masked = logits_of(eng)
  text = '\n'.join(tr.lines)
  assert sum(1 for l in tr.lines if l.startswith('idft_dft_rows<')) == 0, text
  assert sum(1 for l in tr.lines if l.startswith('mask_rows')) == len(layers) - 1, text
  assert any(l.startswith('dft_rows<') for l in tr.lines), text                           # still in the frequency domain
  for b, n in enumerate(lens):
    v = -(-n // 2)
    bound = 1e-5 * max(1.0, float(np.max(np.abs(solo[b]))))
    err = float(np.max(np.abs(masked[b, :v] - solo[b])))
    print('len {}: max |masked - solo| = {:.3e} (bound {:.1e})'.format(n, err, bound))
    assert err < bound
    assert ids[b] == solo_ids[b], b


def test_bf16_masked_equals_solo(small):
  """bf16 activations: masked against solo may differ by roundings to bf16 that fall the other way when another batch shape sums
  in another order.  The yardstick is the arithmetic's own error: the solo bf16 run's distance to the float64 oracle on this
  input, and the masked run may be twice that far from the solo run.
  Measured on MI355X: max |solo - float64| = 5.861e-03 (so the bound is 1.172e-02), max |masked - solo| = 0 (unmasked, the batched
  rows are 3.190e-01 from the solo ones)."""
  eng, x, lens = small['engine']('bf16'), small['x'], SMALL_LENS
  solo = solo_runs(eng, x, lens)
  own = max(float(np.max(np.abs(s - r))) for s, r in zip(solo, small['ref']))
  eng.load_batch(x, lens)
  eng.forward(mask_padding=True)
  masked = logits_of(eng)
  worst = max(float(np.max(np.abs(masked[b, :-(-n // 2)] - solo[b]))) for b, n in enumerate(lens))
  print('bf16: max |solo - float64| = {:.3e}, max |masked - solo| = {:.3e}'.format(own, worst))
  assert own > 0 and worst <= 2 * own
  # the stored bf16 planes are masked
  for i in range(1, len(SMALL_LAYERS)):
    t = eng.X[i]
    full = eng.Xb[i].view(t.batch, t.t_pitch, t.c_pitch).float().cpu().numpy()
    for b, n in enumerate(lens):
      assert not full[b, t.halo + -(-n // 2):].any(), (i, b)
  eng.forward()
  plain = logits_of(eng)
  far = max(float(np.max(np.abs(plain[b, :-(-n // 2)] - solo[b]))) for b, n in enumerate(lens) if n < max(lens))
  print('bf16: unmasked max |batched - solo| = {:.3e}'.format(far))


def test_transcribe_and_align_in_masked_batches(small):
  from speecht_amd import inference
  eng = small['engine']('fp32')
  lens = [57, 90, 120, 121]
  feats = [WL.synthetic_features(80 + i, n, 16).astype(np.float32) for i, n in enumerate(lens)]
  for pipeline in (False, True):
    one = inference.transcribe(eng, feats, batch_size=1, pipeline=pipeline)
    four = inference.transcribe(eng, feats, batch_size=4, mask_padding=True, pipeline=pipeline)
    assert four[0] == one[0] and four[1] == one[1]
  assert any(len(i) for i in one[0])
  ids1, _, spans1 = inference.transcribe(eng, feats, batch_size=1, timestamps=True)
  ids4, _, spans4 = inference.transcribe(eng, feats, batch_size=4, timestamps=True, mask_padding=True)
  assert ids1 == ids4 == one[0]
  assert all(np.array_equal(a, b) for a, b in zip(spans1, spans4))
  labels = [WL.make_labels(7 + i, 6, n // 2) for i, n in enumerate(lens)]
  a1 = inference.align(eng, feats, labels, batch_size=1)
  a4 = inference.align(eng, feats, labels, batch_size=4, mask_padding=True)
  assert a1[2] == a4[2] == [0] * len(lens)
  assert all(np.array_equal(p, q) for p, q in zip(a1[0], a4[0]))
  assert np.allclose(a1[1], a4[1], rtol=1e-5, atol=1e-5)


def test_a_mode_that_cannot_mask_raises(small):
  from speecht_amd._lib import SpeechtHipError
  eng = small['engine']('bf16x6')
  eng.load_batch(small['x'], SMALL_LENS)
  with pytest.raises(SpeechtHipError, match='mask_padding'):
    eng.forward(mask_padding=True)
