"""SpecAugment on the GPU (st_spec_augment_f32 behind ``load_batch(..., augment=...)`` and ``SpeechModel.step``) against its host
form (st_spec_augment_host: the two share csrc/spec_augment_core.h, so every comparison is bit for bit), over the WHOLE input
tensor -- interior, pad channels and halo rows.  The host form itself is held against the float64 specification in
tests/test_spec_augment_cpu.py."""
import numpy as np
import pytest

from tests import workloads as WL

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

IDENTITY = (0, 0, 0, 0, 0, 1.0)
WARP_ONLY = (4, 0, 0, 0, 0, 1.0)
MASKS_ONLY = (0, 5, 8, 6, 8, 1.0)
LD_SMALL = (4, 5, 2, 6, 2, 1.0)          # LD scaled down to utterances of a few dozen frames
POLICIES = [IDENTITY, WARP_ONLY, MASKS_ONLY, LD_SMALL]


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


_ENGINES = {}


def engine(dev, channels):
  from speecht_amd.engine import Wav2LetterEngine
  if channels not in _ENGINES:
    _ENGINES[channels] = Wav2LetterEngine(WL.w2l_layers(channels, width=24, fc=40), device=dev)
  return _ENGINES[channels]


def batch(B, T, C, seed):
  """Noise everywhere, the rows past the lengths included: they must arrive unchanged."""
  return np.random.default_rng(seed).standard_normal((B, T, C)).astype(np.float32)


def device_buffer(eng):
  X0 = eng.shape.X[0]
  torch.cuda.synchronize()
  return X0.buf.cpu().numpy().reshape(X0.batch, X0.t_pitch, X0.c_pitch).copy()


def host_buffer(eng, aug, x, lens):
  """What X[0] must hold: zeros, with the host form's rows and channels written into the interior."""
  from speecht_amd import augmentation as A
  X0 = eng.shape.X[0]
  out = np.zeros((X0.batch, X0.t_pitch, X0.c_pitch), dtype=np.float32)
  _, plan = A.apply_host(aug, x, lens, out=out, halo=X0.halo)
  return out, plan


def same_bits(a, b):
  return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def load(eng, x, lens, aug, staged):
  eng.load_batch(eng.stage_host_batch(x) if staged else x, lens, augment=aug)


@pytest.mark.parametrize('staged', [True, False], ids=['staged', 'numpy'])
@pytest.mark.parametrize('channels', [80, 128, 13])
def test_load_batch_equals_host_form_on_the_whole_input_tensor(dev, channels, staged):
  from speecht_amd import augmentation as A
  eng = engine(dev, channels)
  lens = [37, 20, 1]
  x = batch(3, 37, channels, seed=channels)
  load(eng, x, lens, None, staged)
  plain = device_buffer(eng)
  assert same_bits(plain[:, eng.shape.X[0].halo:eng.shape.X[0].halo + 37, :channels], x)
  for n, policy in enumerate(POLICIES):
    aug = A.SpecAugment(policy, seed=77 + n, draw_ids=[1000 * n + 5, 2 ** 40 + n, -3 - n])
    load(eng, x, lens, aug, staged)
    got = device_buffer(eng)
    want, plan = host_buffer(eng, aug, x, lens)
    assert same_bits(got, want), (policy, int(np.sum(got.view(np.int32) != want.view(np.int32))))
    assert np.array_equal(eng.augment_plan.cpu().numpy(), plan) and plan.shape == (3, 2 + 2 * (policy[2] + policy[4]))
    assert np.array_equal(plan, A.plan_host(aug, lens, channels))
    if policy == IDENTITY:
      assert same_bits(got, plain)                   # the plain copy, bit for bit
    else:
      assert not same_bits(got, plain)
    if policy[0]:
      assert plan[0, 0] > 0 and plan[1, 0] > 0 and plan[2, 0] == 0          # lengths 37 and 20 >= 2 W + 2, length 1 is not warped


def test_rows_one_past_the_workgroups(dev):
  """frames = 2 workgroups' rows + 1: the last workgroup of every utterance owns a single row."""
  from speecht_amd import augmentation as A
  T = 2 * A.ROWS_PER_WORKGROUP + 1
  eng = engine(dev, 80)
  lens = [T, A.ROWS_PER_WORKGROUP + 1]
  x = batch(2, T, 80, seed=5)
  for policy in (WARP_ONLY, LD_SMALL):
    aug = A.SpecAugment(policy, seed=9, draw_ids=[7, 8])
    eng.load_batch(x, lens, augment=aug)
    want, plan = host_buffer(eng, aug, x, lens)
    assert same_bits(device_buffer(eng), want)
    assert np.array_equal(eng.augment_plan.cpu().numpy(), plan)


def test_shape_reentry_keeps_pad_channels_and_halos_clean(dev):
  from speecht_amd import augmentation as A
  eng = engine(dev, 13)
  lens = [37, 20, 1]
  x = batch(3, 37, 13, seed=1)
  first = A.SpecAugment(LD_SMALL, seed=3, draw_ids=[0, 1, 2])
  eng.load_batch(x, lens, augment=first)
  assert same_bits(device_buffer(eng), host_buffer(eng, first, x, lens)[0])
  eng.load_batch(batch(2, 64, 13, seed=2), [64, 50])
  again = first.at([10, 11, 12])
  eng.load_batch(x, lens, augment=again)
  want, plan = host_buffer(eng, again, x, lens)
  assert same_bits(device_buffer(eng), want)
  assert not np.array_equal(plan, host_buffer(eng, first, x, lens)[1])


def test_bad_augment_arguments_raise_before_any_launch(dev):
  from speecht_amd import augmentation as A
  eng = engine(dev, 13)
  x = batch(3, 37, 13, seed=1)
  with pytest.raises(ValueError):
    eng.load_batch(x, [37, 20, 38], augment=A.SpecAugment(LD_SMALL, 0, [0, 1, 2]))
  with pytest.raises(ValueError):
    eng.load_batch(x, [37, 20, 1], augment=A.SpecAugment(LD_SMALL, 0, [0, 1]))
  with pytest.raises(ValueError):
    eng.load_batch(x, [37, 20, 1], augment=A.SpecAugment(LD_SMALL, 0))


# ---- through SpeechModel.step, on the model of tests/test_gpu_api.py --------------------------------------------------------

FRAMES = [121, 100, 90, 121]


def make_model(tmp_path, name, spec_augment=None):
  from speecht_amd.speech_input import Coordinator, InputBatchLoader
  from speecht_amd.speech_model import Wav2LetterModel
  x, seq, labels = WL.make_batch(FRAMES, 16, seed=0)

  def gen():
    while True:
      for i in range(len(FRAMES)):
        yield x[i, :seq[i]], labels[i]
  loader = InputBatchLoader(16, len(FRAMES), gen)
  coord = Coordinator()
  loader.start_threads(None, coord)
  model = Wav2LetterModel(loader, 16, 29)
  model.add_training_ops(learning_rate=1e-3, spec_augment=spec_augment)
  model.add_decoding_ops()
  model.finalize(str(tmp_path / 'log'), name, 'train')
  model.init_seed = 11
  return model, coord, x.astype(np.float32), seq


def test_step_augments_updating_steps_only(dev, tmp_path):
  from speecht_amd import augmentation as A
  from speecht_amd.speech_model import Session
  aug = A.SpecAugment((8, 5, 2, 12, 2, 1.0), seed=21)
  model, coord, x, seq = make_model(tmp_path, 'a', aug)
  other, coord2, _, _ = make_model(tmp_path, 'b')
  try:
    with Session(dev) as sess:
      model.init_session(sess)
      other.init_session(sess)
      assert torch.equal(model.engine.params, other.engine.params)
      # evaluation and decoding: the features as they are
      model.step(sess, loss=True, update=False, decode=True)
      X0 = model.engine.shape.X[0]
      assert same_bits(X0.interior().cpu().numpy(), x)
      # an updating step: the loss of the host-form-augmented batch fed to a model without a policy, bit for bit
      ids = A.draw_ids(0, len(FRAMES))
      assert ids.tolist() == [0, 1, 2, 3]
      loss = model.step(sess)[0]
      fed, plan = A.apply_host(aug.at(ids), x, seq)
      assert not same_bits(np.ascontiguousarray(fed), x)
      assert np.array_equal(model.engine.augment_plan.cpu().numpy(), plan)
      assert same_bits(model.engine.shape.X[0].interior().cpu().numpy(), np.ascontiguousarray(fed))
      want = other.step(sess, feed_dict={other.inputs: np.ascontiguousarray(fed), other.sequence_lengths: seq})[0]
      assert np.float32(loss).tobytes() == np.float32(want).tobytes(), (loss, want)
      plain = other.step(sess, update=False)[0]
      assert np.isfinite(plain)
      # the next step draws with the ids of global step 1
      model.step(sess)
      assert np.array_equal(model.engine.augment_plan.cpu().numpy(), A.plan_host(aug.for_step(1, len(FRAMES)), seq, 16))
  finally:
    coord.request_stop()
    coord2.request_stop()


def test_same_seed_same_losses_other_seed_other_loss(dev, tmp_path):
  from speecht_amd import augmentation as A
  from speecht_amd.speech_model import Session

  def run(name, seed):
    model, coord, _, _ = make_model(tmp_path, name, A.SpecAugment((8, 5, 2, 12, 2, 1.0), seed=seed))
    try:
      with Session(dev) as sess:
        model.init_session(sess)
        return [np.float32(model.step(sess)[0]).tobytes() for _ in range(3)]
    finally:
      coord.request_stop()
  first, second, third = run('s1', 5), run('s2', 5), run('s3', 6)
  assert first == second
  assert first[0] != third[0]
