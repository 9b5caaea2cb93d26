"""The LM-scored CTC prefix beam search on the GPU (st_ctc_beam_search_decode_lm, ctc_beam_kernel<.., LM = true) against the
float64 specification of tests/lm_oracle.py: identical label sequences, log-probabilities (LM terms included) within 1e-4;
with every weight 0 bit for bit the LM-free kernel; and the layers above it -- engine, pipelined transcribe, model, CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import w2l_oracle as O
from tests import lm_oracle as L
from tests import workloads as WL
from tests.test_lm_oracle_cpu import word_logits

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, 'tests', 'golden', 'lm_tiny.arpa')
SENTENCE_WORDS = ['the', 'cat', 'sat', 'on', 'mat', 'dog', 'a', "it's"]


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def _engine(dev, logits, lens):
  from speecht_amd.engine import Wav2LetterEngine
  T, B, C = logits.shape
  eng = Wav2LetterEngine([(1, 1, 16, C, False)], device=dev)
  eng.load_batch(np.zeros((B, T, 16)), [T] * B)
  eng.X[-1].interior().copy_(torch.as_tensor(np.transpose(logits, (1, 0, 2)).astype(np.float32)))
  eng.ctc_lens = torch.as_tensor(np.asarray(lens).astype(np.int32)).to(dev)
  return eng


_MODELS = {}


def _model(tmp_dir, order):
  """order 3: the hand-written model; others: a seeded random model whose vocabulary holds the sentence words."""
  from speecht_amd.language_model import LanguageModel
  if order == 3:
    return LanguageModel.load(TINY), L.ArpaModel.load(TINY)
  if order not in _MODELS:
    text = L.random_arpa(100 + order, 150, [400, 300, 200, 100][:order - 1], extra_words=SENTENCE_WORDS)
    path = os.path.join(tmp_dir, 'r{}.arpa'.format(order))
    with open(path, 'w') as f:
      f.write(text)
    _MODELS[order] = (LanguageModel.load(path), L.ArpaModel(text))
  return _MODELS[order]


def _cases(seed):
  rng = np.random.default_rng(seed)
  T, B, C = 80, 5, 29
  logits = rng.standard_normal((T, B, C)) * 2.0
  w = word_logits('the cat sat on the mat', rng, frames_per_char=2, gap=1, noise=1.0, peak=3.0)
  logits[:len(w), 1] = w
  logits[:, 2, 28] += 3.0                                  # mostly blanks
  lens = [80, len(w), 77, 0, 1]
  return logits.astype(np.float32), lens


@pytest.mark.parametrize('beam', [1, 16, 64, 100, 128])
@pytest.mark.parametrize('order', [1, 2, 3, 4, 5])
def test_lm_beam_search_matches_the_oracle(dev, tmp_path_factory, beam, order):
  lm, ref = _model(str(tmp_path_factory.getbasetemp()), order)
  logits, lens = _cases(10 * beam + order)
  transform = 'log10_softmax' if (beam + order) % 2 else None
  eng = _engine(dev, logits, lens)
  from speecht_amd._lib import launch_trace
  with launch_trace() as tr:
    ids, logp = eng.lm_beam_search_decode(lm, beam, input_transform=transform)
  assert any(l.startswith('ctc_beam_lm<') and 'order={}'.format(order) in l for l in tr.lines), tr.lines
  ref_ids, ref_logp = L.lm_beam_search_decode(logits.astype(np.float64), lens, ref, beam, transform)
  assert ids == ref_ids
  np.testing.assert_allclose(logp, ref_logp, rtol=1e-4, atol=1e-4)
  assert ids[3] == []


def test_reference_operating_point_on_long_form(dev):
  """Beam 100 on T' = 1501 (30 s), the reference's input transform and weights: the ids match the oracle."""
  from speecht_amd.language_model import LanguageModel
  rng = np.random.default_rng(1501)
  w = word_logits("the cat sat on the mat a dog ran in the house it's a hat ", rng, frames_per_char=3, gap=2, noise=1.5, peak=3.0)
  reps = int(np.ceil(1501 / len(w)))
  logits = np.tile(w, (reps, 1))[:1501][:, None, :].astype(np.float32)
  lm, ref = LanguageModel.load(TINY), L.ArpaModel.load(TINY)
  eng = _engine(dev, logits, [1501])
  ids, logp = eng.lm_beam_search_decode(lm, 100)
  ref_ids, ref_logp = L.lm_beam_search_decode(logits.astype(np.float64), [1501], ref, 100, 'log10_softmax')
  assert ids == ref_ids
  np.testing.assert_allclose(logp, ref_logp, rtol=1e-4)


@pytest.mark.parametrize('beam', [16, 100])
def test_zero_weights_equal_the_lm_free_kernel_bit_for_bit(dev, beam):
  from speecht_amd.language_model import LanguageModel
  logits, lens = _cases(beam)
  eng = _engine(dev, logits, lens)
  lm = LanguageModel.load(TINY)
  for transform in (None, 'log10_softmax'):
    a_ids, a_lp = eng.lm_beam_search_decode(lm, beam, transform, lm_weight=0.0, word_count_weight=0.0, valid_word_count_weight=0.0)
    b_ids, b_lp = eng.beam_search_decode(beam, transform)
    assert a_ids == b_ids and np.array_equal(a_lp, b_lp)


def test_the_language_model_decides_the_spelling(dev):
  from speecht_amd.language_model import LanguageModel
  rng = np.random.default_rng(7)
  x = word_logits('the kat', rng, noise=0.3)
  k, c = L.LETTERS.index('k'), L.LETTERS.index('c')
  for t in range(len(x)):
    if x[t].argmax() == k:
      x[t, c] = x[t, k] - 0.5
  eng = _engine(dev, x[:, None, :].astype(np.float32), [len(x)])
  plain, _ = eng.beam_search_decode(16)
  with_lm, _ = eng.lm_beam_search_decode(LanguageModel.load(TINY), 16, input_transform=None)
  assert L.ids_to_text(plain[0]) == 'the kat' and L.ids_to_text(with_lm[0]) == 'the cat'


def test_pipelined_transcribe_with_a_language_model_equals_the_serial_loop(dev):
  from speecht_amd.engine import Wav2LetterEngine
  from speecht_amd.inference import transcribe
  layers = WL.w2l_layers(16, width=40, fc=72)
  params = WL.xavier_params(layers, seed=21, bias_range=0.3)
  params[-1] = (params[-1][0] * 12.0, params[-1][1] * 4.0)
  rng = np.random.default_rng(8)
  lengths = rng.integers(60, 260, 13).tolist()
  feats = [WL.synthetic_features(300 + i, t, 16).astype(np.float32) for i, t in enumerate(lengths)]
  eng = Wav2LetterEngine(layers, device=dev)
  eng.set_weights(params)
  opts = dict(lm_weight=2.0, valid_word_count_weight=1.0)
  a, _ = transcribe(eng, feats, batch_size=4, pipeline=True, beam_width=32, language_model=TINY, lm_options=opts)
  b, _ = transcribe(eng, feats, batch_size=4, pipeline=False, beam_width=32, language_model=TINY, lm_options=opts)
  assert a == b and any(len(s) > 0 for s in a)
  # one batch against the oracle on the device's own logits
  idx = list(range(4))
  x, seq, _ = O.pad_batch([feats[i].astype(np.float64) for i in idx], 16)
  eng.load_batch(x, seq)
  eng.forward()
  torch.cuda.synchronize()
  logits = eng.logits_time_major().cpu().numpy().astype(np.float64)
  ref_ids, _ = L.lm_beam_search_decode(logits, seq // 2, L.ArpaModel.load(TINY), 32, 'log10_softmax', **opts)
  serial, _ = transcribe(eng, [feats[i] for i in idx], batch_size=4, bucket=False, pipeline=False, beam_width=32,
                         language_model=TINY, lm_options=opts)
  assert serial == ref_ids


def test_a_handle_without_a_copy_on_the_device_is_refused(dev):
  """The decoder reads the tables' copy on its stream's device: a handle never uploaded there is an error, not a fault."""
  import ctypes
  from speecht_amd import _lib
  from speecht_amd.language_model import LanguageModel
  lm = LanguageModel(TINY)                                  # a fresh handle, not uploaded anywhere
  logits, lens = _cases(3)
  eng = _engine(dev, logits, lens)
  lib = _lib.load()
  B = eng.dec_lens.numel()
  ws = torch.empty(lib.st_ctc_beam_ws(B, eng.t_out, 16) // 4 + 16, dtype=torch.int32, device=dev)
  eng._wait_uploads()
  with pytest.raises(_lib.SpeechtHipError, match='not on device'):
    _lib.call('st_ctc_beam_search_decode_lm', eng.X[-1].ref, eng._ptr(eng.ctc_lens), 16, 0, lm._handle, ctypes.c_float(0.8),
              ctypes.c_float(0.0), ctypes.c_float(2.3), ctypes.c_float(-1000.0), eng._ptr(eng.dec_ids), eng.t_out,
              eng._ptr(eng.dec_lens), eng._ptr(eng.dec_score), eng._ptr(ws), ws.numel() * 4, eng.stream_ptr)
  ids, _ = eng.lm_beam_search_decode(lm, 16)               # the engine uploads to its own device first
  assert len(ids) == B


def test_engines_on_two_devices_share_one_model():
  """One cached model, engines on cuda:0 and cuda:1: each decodes with a copy on its own device, with the same result."""
  if torch.cuda.device_count() < 2:
    pytest.skip('needs two GPUs')
  from speecht_amd.language_model import LanguageModel
  logits, lens = _cases(4)
  lm = LanguageModel.load(TINY)
  got = [_engine('cuda:{}'.format(d), logits, lens).lm_beam_search_decode(lm, 16) for d in (1, 0)]
  assert got[0][0] == got[1][0] and np.array_equal(got[0][1], got[1][1])


def test_model_step_decodes_with_the_language_model(dev, tmp_path):
  """SpeechModel.add_decoding_ops(language_model=...) + step(decode=True): beam 100 on log10(softmax + 1e-8) with the
  reference's weights -- the oracle's search on the device's own logits; a non-ARPA path still raises NotImplementedError."""
  from speecht_amd.speech_input import SingleInputLoader
  from speecht_amd.speech_model import Session, Wav2LetterModel
  loader = SingleInputLoader(16)
  model = Wav2LetterModel(loader, 16, 29)
  model.add_training_ops()
  model.add_decoding_ops(language_model=TINY)
  model.finalize(str(tmp_path), 'r', 'record')
  feats = WL.synthetic_features(5, 91, 16)
  with Session(dev) as sess:
    model.init_session(sess)
    loader.set_input(feats)
    decoded, = model.step(sess, loss=False, update=False, decode=True)
    logits = model.engine.logits_time_major().cpu().numpy().astype(np.float64)
  ref_ids, _ = L.lm_beam_search_decode(logits, [91 // 2], L.ArpaModel.load(TINY), 100, 'log10_softmax')
  assert decoded[0].values.tolist() == ref_ids[0]
  (tmp_path / 'kenlm').mkdir()
  (tmp_path / 'kenlm' / 'lm.binary').write_bytes(bytes(16))
  with pytest.raises(NotImplementedError):
    model.add_decoding_ops(language_model=str(tmp_path / 'kenlm'))


def test_cli_evaluate_with_a_language_model(dev, tmp_path):
  """`speecht-cli evaluate --language-model lm_tiny.arpa --lm-weight 3.0` on the configs[0] plumbing (batch 4 of 2 s clips, a
  3-step checkpoint) prints what the oracle's LM search gives at lm_weight 3.0 on the logits of that checkpoint.  The four test
  utterances are one clip, so every row of the evaluation batch has the logits of the clip alone, whatever the batch order."""
  from speecht_amd.speech_input import SingleInputLoader
  from speecht_amd.speech_model import Session, Wav2LetterModel
  from tests.test_gpu_api import write_wav
  data = tmp_path / 'data'
  for split in ('train', 'test'):
    (data / split).mkdir(parents=True)
    lines = []
    for i in range(4):
      uid = 'spk-{}-{:04d}'.format(split, i)
      write_wav(str(data / split / (uid + '.wav')), O.synthetic_audio(i if split == 'train' else 0, 32000))
      lines.append('{} {}'.format(uid, 'THE CAT SAT ON THE MAT'))
    (data / split / 'x.trans.txt').write_text('\n'.join(lines) + '\n')
  cli = [sys.executable, os.path.join(ROOT, 'speecht-cli')]
  common = ['--data-dir', str(data), '--train-dir', str(tmp_path / 'train'), '--log-dir', str(tmp_path / 'log'),
            '--run-name', 'ci', '--batch-size', '4']
  run = lambda args: subprocess.run(cli + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
  r = run(['preprocess'] + common)
  assert r.returncode == 0, r.stdout + r.stderr
  r = run(['train'] + common + ['--steps-per-checkpoint', '3', '--max-steps', '3', '--learning-rate', '1e-3'])
  assert r.returncode == 0, r.stdout + r.stderr
  r = run(['evaluate', '--step-count', '1', '--no-save', '--pair-by-row', '--language-model', TINY, '--lm-weight', '3.0'] + common)
  assert r.returncode == 0, r.stdout + r.stderr
  printed = [l.split('decoded: ', 1)[1] if 'decoded: ' in l else '' for l in r.stdout.splitlines() if l.startswith('decoded:')]
  assert len(printed) == 4, r.stdout
  # the same batch in-process -- four rows of the clip through the restored checkpoint -- and the oracle's search on its logits
  feats = np.load(str(data / 'preprocessed-power' / 'test' / 'spk-test-0000.npz'))['audio_fragments']
  loader = SingleInputLoader(feats.shape[1])
  model = Wav2LetterModel(loader, feats.shape[1], 29)
  model.add_training_ops()
  model.add_decoding_ops()
  model.finalize(str(tmp_path / 'log2'), 'r', 'record')
  with Session(dev) as sess:
    model.restore(sess, str(tmp_path / 'train' / 'ci'))
    eng = model.engine
    eng.load_batch(np.stack([feats] * 4).astype(np.float32), [len(feats)] * 4)
    eng.forward()
    logits = eng.logits_time_major().cpu().numpy().astype(np.float64)
    lens = eng.ctc_lens.cpu().numpy()
  ref3, _ = L.lm_beam_search_decode(logits[:, :1], lens[:1], L.ArpaModel.load(TINY), 100, 'log10_softmax', lm_weight=3.0)
  ref08, _ = L.lm_beam_search_decode(logits[:, :1], lens[:1], L.ArpaModel.load(TINY), 100, 'log10_softmax', lm_weight=0.8)
  assert printed == [L.ids_to_text(ref3[0])] * 4, (printed, L.ids_to_text(ref3[0]))
  assert ref3 != ref08                                     # (so the printed strings also pin that --lm-weight arrived)
