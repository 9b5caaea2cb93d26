"""CTC word confidences on the GPU: st_ctc_word_conf_f32 bit for bit against its host form (st_ctc_word_conf_host -- the two share
their arithmetic, csrc/ctc_conf_core.h; the host form is held to the float64 oracle within 1e-9 in tests/test_conf_cpu.py, and
the kernel therefore too), through every states-per-lane dispatch and up to 1 501 frames; `engine.word_confidence`,
`transcribe(confidence=True)`, `transcribe_files(confidence=True)` and the command line on top of it."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import align_oracle as AO
from tests import conf_oracle as CO
from tests import workloads as WL
from tests.test_conf_cpu import GATE, SPACE, C, check_against_oracle, dispatch_cases, host_conf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
GOLDEN_FLAC = os.path.join(GOLDEN, '1089-134686-0037.flac')
TINY_LM = os.path.join(GOLDEN, 'lm_tiny.arpa')
C_PITCH = 32


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def device_conf(dev, logits, labels, seq_lens, space_id=SPACE, max_label_len=None, spans=None, garbage=True):
  """st_ctc_word_conf_f32 on a dense [B, T, C] batch laid out as padded NWC (halo 0, c_pitch 32): the pitch columns hold 1e30,
  the rows past seq_lens garbage, a sentinel sits behind every output and the inputs must come back unchanged
  -> (log_prob [B], log_conf [n_words], status [B], spans [n_words, 3])."""
  from speecht_amd import _lib
  from speecht_amd._lib import Tensor3
  lib = _lib.load()
  logits = np.array(logits, dtype=np.float32)
  B, T, Cc = logits.shape
  lens = np.asarray(seq_lens, dtype=np.int32)
  if garbage:
    junk = np.random.default_rng(1).choice(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3.0], np.float32), size=logits.shape)
    for b in range(B):
      if 0 <= lens[b] <= T:
        logits[b, lens[b]:] = junk[b, lens[b]:]
  ids, offs = CO.csr(labels)
  spans = CO.batch_spans(labels, space_id) if spans is None else np.ascontiguousarray(spans, dtype=np.int32).reshape(-1, 3)
  W = len(spans)
  max_len = max([len(l) for l in labels] + [0]) if max_label_len is None else max_label_len
  x = torch.full((B, T, C_PITCH), 1e30, dtype=torch.float32, device=dev)      # the pitch columns must never be read
  x[:, :, :Cc] = torch.as_tensor(logits)
  x0 = x.clone()
  to = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
  d_ids, d_offs, d_lens = to(ids), to(offs), to(lens)
  d_spans = to(np.concatenate([spans.reshape(-1), np.full(3, -9, np.int32)]))
  log_prob = torch.full((B + 1,), 7.0, dtype=torch.float64, device=dev)
  log_conf = torch.full((W + 1,), 7.0, dtype=torch.float64, device=dev)
  status = torch.full((B + 1,), -7, dtype=torch.int32, device=dev)
  need = lib.st_ctc_word_conf_ws(B, T, max_len, B + W)
  ws = torch.full((need // 4 + 8,), -3, dtype=torch.int32, device=dev)
  P = lambda t: ctypes.c_void_p(t.data_ptr())
  desc = Tensor3(x.data_ptr(), B, T, Cc, 0, T, C_PITCH)
  _lib.call('st_ctc_word_conf_f32', ctypes.byref(desc), P(d_ids), P(d_offs), P(d_lens), max_len, space_id, P(d_spans), W,
            P(log_prob), P(log_conf), P(status), P(ws), need, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
  torch.cuda.synchronize()
  # nothing written past the outputs or the workspace, no input touched
  assert log_prob[-1].item() == 7.0 and log_conf[-1].item() == 7.0 and status[-1].item() == -7
  assert (ws[need // 4:] == -3).all()
  assert torch.equal(x.view(torch.int32), x0.view(torch.int32))
  assert (d_ids.cpu().numpy() == ids).all() and (d_offs.cpu().numpy() == offs).all() and (d_lens.cpu().numpy() == lens).all()
  assert (d_spans.cpu().numpy()[:3 * W] == spans.reshape(-1)).all() and (d_spans.cpu().numpy()[3 * W:] == -9).all()
  return log_prob[:B].cpu().numpy(), log_conf[:W].cpu().numpy(), status[:B].cpu().numpy(), spans


def same_bits(dev_res, host_res):
  return all((bits(a) == bits(b)).all() for a, b in zip(dev_res[:2], host_res[:2])) and (dev_res[2] == host_res[2]).all()


@pytest.mark.parametrize('planted', [False, True], ids=['random', 'planted'])
def test_kernel_equals_the_host_form_bit_for_bit(dev, planted):
  for logits, labs, lens, xs in dispatch_cases(planted):
    got = device_conf(dev, logits, labs, lens)
    want = host_conf(logits, labs, lens)
    assert got[2].tolist() == [0, 0, 0, 0, 1]
    assert same_bits(got, want), (len(labs[0]), np.abs(got[1] - want[1]).max())
    assert np.isfinite(got[0][:4]).all() and got[0][4] == -np.inf
    assert np.isnan(got[1][got[3][:, 0] == 4]).all() and (got[1][got[3][:, 0] != 4] <= 0.0).all()
  # the smallest dispatch batch against the oracle itself (the others: through the host form, tests/test_conf_cpu.py)
  logits, labs, lens, xs = dispatch_cases(planted)[0]
  assert max(check_against_oracle(xs, labs, *device_conf(dev, logits, labs, lens))) <= GATE


def test_small_launches_and_refusals(dev):
  rng = np.random.default_rng(21)
  # B = 1 with one word: the smallest launch
  x = AO.random_logits(rng, 9, C, 1.0)
  got = device_conf(dev, x[None], [[3, 4]], [9])
  assert same_bits(got, host_conf(x[None], [[3, 4]], [9])) and len(got[1]) == 1 and got[1][0] < 0.0
  assert max(check_against_oracle([x], [[3, 4]], *got)) <= GATE
  # n_words = 0; an utterance without frames
  labs = [[], [SPACE], []]
  xs = [AO.random_logits(rng, 12, C), AO.random_logits(rng, 5, C), AO.random_logits(rng, 0, C)]
  logits, lens = AO.pad_batch(xs)
  got = device_conf(dev, logits, labs, lens)
  assert same_bits(got, host_conf(logits, labs, lens)) and len(got[1]) == 0 and got[2].tolist() == [0, 0, 0] and got[0][2] == 0.0
  assert abs(got[0][0] - AO.log_softmax64(xs[0])[:, C - 1].sum()) <= GATE
  # one refused utterance leaves its neighbours alone
  labs = [[1, 2, SPACE, 3, 3], [4, 4, 4, SPACE, 5], [6, SPACE, 7]]
  xs = [AO.random_logits(rng, 30, C), AO.random_logits(rng, 6, C), AO.random_logits(rng, 17, C)]
  logits, lens = AO.pad_batch(xs)
  got = device_conf(dev, logits, labs, lens)
  assert same_bits(got, host_conf(logits, labs, lens)) and got[2].tolist() == [0, 1, 0]
  assert got[0][1] == -np.inf and np.isnan(got[1][2:4]).all() and np.isfinite(got[1][[0, 1, 4, 5]]).all()
  for b in (0, 2):
    alone = device_conf(dev, logits[b:b + 1], [labs[b]], lens[b:b + 1], max_label_len=5)
    assert bits(alone[0])[0] == bits(got[0])[b] and (bits(alone[1]) == bits(got[1][got[3][:, 0] == b])).all()
  # lengths outside 0 .. frames and a label beyond the dispatch (max_label_len 12 holds 31) are refused per utterance
  lens_bad = lens.copy()
  lens_bad[2] = 31
  labs_long = [list(range(20)) + [SPACE] + list(range(20))] + labs[1:]
  got = device_conf(dev, logits, labs_long, lens_bad, max_label_len=12)
  assert got[2].tolist() == [1, 1, 1] and np.isnan(got[1]).all() and (got[0] == -np.inf).all()
  assert same_bits(got, host_conf(logits, labs_long, lens_bad, max_label_len=12))
  # spans that are no word runs, P(l) = 0, single infinite logits: the host form's bits, nothing written elsewhere
  wild = [(0, 0, 5), (0, 2, 3), (0, 3, 2), (0, -1, 2), (0, 0, 6), (7, 0, 1), (-1, 0, 1), (1, 0, 1), (2, 1, 2)]
  got = device_conf(dev, logits, labs, lens, spans=wild)
  assert same_bits(got, host_conf(logits, labs, lens, spans=wild)) and np.isnan(got[1][2:8]).all()
  dead = np.array(logits)
  dead[0, :, 2] = -np.inf
  dead[2, 3, 6] = dead[2, 5, C - 1] = -np.inf
  got = device_conf(dev, dead, labs, lens)
  assert same_bits(got, host_conf(dead, labs, lens)) and got[0][0] == -np.inf and (got[1][:2] == -np.inf).all()
  assert np.isfinite(got[1][4:]).all()


def test_more_jobs_than_one_wave_of_blocks(dev):
  """8 utterances x 40 short words at T = 140: 328 jobs in one call."""
  rng = np.random.default_rng(22)
  labs = []
  for b in range(8):
    lab = []
    for w in range(40):
      lab += ([SPACE] if w else []) + [int(rng.integers(0, 26))]
    labs.append(lab)
  xs = [AO.planted_logits(rng, lab, int(rng.integers(100, 141)), C, boost=4.0)[0] for lab in labs]
  logits, lens = AO.pad_batch(xs, 140)
  got = device_conf(dev, logits, labs, lens)
  assert len(got[1]) == 320 and (got[2] == 0).all()
  assert same_bits(got, host_conf(logits, labs, lens))
  again = device_conf(dev, logits, labs, lens, garbage=False)          # run to run, and whatever the padding rows hold
  assert same_bits(again, got)
  assert max(check_against_oracle(xs[:2], labs[:2], got[0][:2], got[1][:80], got[2][:2], got[3][:80])) <= GATE


def _small_engine(dev, scale=(12.0, 4.0)):
  from speecht_amd.engine import Wav2LetterEngine
  layers = WL.w2l_layers(16, width=40, fc=72)
  params = WL.xavier_params(layers, seed=21, bias_range=0.3)
  params[-1] = (params[-1][0] * scale[0], params[-1][1] * scale[1])
  eng = Wav2LetterEngine(layers, device=dev)
  eng.set_weights(params)
  return eng


def test_engine_word_confidence_equals_the_oracle(dev):
  eng = _small_engine(dev)
  lengths = [260, 201, 124, 77]
  feats = [WL.synthetic_features(300 + i, t, 16).astype(np.float32) for i, t in enumerate(lengths)]
  x = np.zeros((len(feats), max(lengths), 16), dtype=np.float32)
  for b, f in enumerate(feats):
    x[b, :f.shape[0]] = f
  eng.load_batch(x, lengths)
  eng.forward()
  ids, _ = eng.greedy_decode()
  assert any(len(CO.split_words(s, SPACE)) >= 1 for s in ids)
  conf, log_prob, status = eng.word_confidence(ids)
  logits = eng.logits_time_major().cpu().numpy().transpose(1, 0, 2)
  assert log_prob.shape == (4, 1) and log_prob.dtype == np.float64 and (status == 0).all()
  for b, lab in enumerate(ids):
    ref = CO.word_conf64(logits[b, :lengths[b] // 2], lab, SPACE)
    assert conf[b].dtype == np.float64 and conf[b].shape == ref['log_conf'].shape
    assert abs(log_prob[b, 0] - ref['log_prob']) <= GATE
    assert len(conf[b]) == 0 or np.abs(conf[b] - ref['log_conf']).max() <= GATE
  # refused on the host: wrong batch, ids outside the classes, too long
  with pytest.raises(ValueError):
    eng.word_confidence(ids[:2])
  with pytest.raises(ValueError):
    eng.word_confidence([[28]] + ids[1:])
  with pytest.raises(ValueError):
    eng.word_confidence([[1] * 512] + ids[1:])
  # a transcript that does not fit is a status, and the others are scored as before
  conf2, lp2, st2 = eng.word_confidence([[1, 2] * 40] + ids[1:3] + [[3] * 39])
  assert st2.tolist() == [0, 0, 0, 1] and lp2[3, 0] == -np.inf and np.isnan(conf2[3]).all()
  assert all((bits(conf2[b]) == bits(conf[b])).all() for b in (1, 2)) and (bits(lp2[1:3]) == bits(log_prob[1:3])).all()


def test_transcribe_with_confidence_keeps_the_ids(dev):
  from speecht_amd.inference import align, transcribe
  eng = _small_engine(dev)
  rng = np.random.default_rng(8)
  lengths = rng.integers(60, 260, 9).tolist()
  feats = [WL.synthetic_features(300 + i, t, 16).astype(np.float32) for i, t in enumerate(lengths)]
  for decode in ({}, dict(language_model=TINY_LM, beam_width=32, lm_options=dict(lm_weight=2.0))):
    ids, texts = transcribe(eng, feats, batch_size=4, **decode)
    ids_c, texts_c, conf = transcribe(eng, feats, batch_size=4, confidence=True, **decode)
    ids_t, texts_t, spans, conf_t = transcribe(eng, feats, batch_size=4, confidence=True, timestamps=True, **decode)
    assert ids_c == ids and texts_c == texts and ids_t == ids and texts_t == texts, decode
    assert any(len(t.split()) >= 1 for t in texts)
    for i, c in enumerate(conf):
      assert set(c) == {'log_prob', 'words'} and len(c['words']) == len(texts[i].split())
      assert all(0.0 <= w <= 1.0 for w in c['words']) and c['log_prob'] <= 0.0
      assert conf_t[i] == c and spans[i].shape == (len(ids[i]), 2)
  # the confidences of one utterance alone: the oracle's on the logits the engine produced
  i = max(range(len(ids)), key=lambda k: len(ids[k]))
  _, _, one = transcribe(eng, [feats[i]], batch_size=1, confidence=True)
  logits = eng.logits_time_major().cpu().numpy()[:, 0]
  lab = transcribe(eng, [feats[i]], batch_size=1)[0][0]
  ref = CO.word_conf64(logits[:lengths[i] // 2], lab, SPACE)
  assert abs(one[0]['log_prob'] - ref['log_prob']) <= GATE and np.abs(np.log(one[0]['words']) - ref['log_conf']).max() <= 1e-9
  # inference.align with confidence: of the given labels
  res = align(eng, feats, ids, batch_size=4, confidence=True)
  assert len(res) == 4 and all(s == 0 for s in res[2])
  assert all(a == b for a, b in zip(res[3], conf))
  assert transcribe(eng, [], confidence=True) == ([], [], []) and transcribe(eng, [], confidence=True, timestamps=True) == ([], [], [], [])


def _golden_model(tmp_path):
  from speecht_amd.speech_input import SingleInputLoader
  from speecht_amd.speech_model import Wav2LetterModel
  loader = SingleInputLoader(128)
  model = Wav2LetterModel(loader, 128, 29)
  model.add_training_ops()
  model.add_decoding_ops()
  model.finalize(str(tmp_path / 'log'), 'r', 'record')
  model.init_seed = 1234
  return model


def test_files_and_command_line_on_the_golden_flac(dev, tmp_path):
  import json
  import shutil
  import subprocess
  import sys
  from speecht_amd import alignment, transcription
  from speecht_amd.speech_model import Session
  model = _golden_model(tmp_path)
  train = tmp_path / 'train'
  (train / 'run').mkdir(parents=True)
  with Session(dev) as sess:
    model.init_session(sess)
    model.saver.save(sess, str(train / 'run' / 'speechT'), global_step=model.global_step)
    plain = transcription.transcribe_files(model.engine, [GOLDEN_FLAC], timestamps=True)
    res = transcription.transcribe_files(model.engine, [GOLDEN_FLAC], timestamps=True, confidence=True)
    logits = model.engine.logits_time_major().cpu().numpy()[:, 0]
    lm = transcription.transcribe_files(model.engine, [GOLDEN_FLAC], language_model=TINY_LM, beam_width=32)
    lm_c = transcription.transcribe_files(model.engine, [GOLDEN_FLAC], language_model=TINY_LM, beam_width=32, confidence=True)
    transcripts = alignment.find_transcripts([GOLDEN_FLAC])
    al = alignment.align_files(model.engine, [GOLDEN_FLAC], transcripts, confidence=True)
    al_plain = alignment.align_files(model.engine, [GOLDEN_FLAC], transcripts)
  r, p = res[0], plain[0]
  assert r['error'] is None and r['ids'] == p['ids'] and r['text'] == p['text'] and (r['spans'] == p['spans']).all()
  assert 'confidence' not in p and lm_c[0]['ids'] == lm[0]['ids'] and 'confidence' in lm_c[0]
  ref = CO.word_conf64(logits[:r['frames']], r['ids'], SPACE)
  assert abs(r['confidence']['log_prob'] - ref['log_prob']) <= GATE
  assert len(r['confidence']['words']) == len(r['text'].split())
  if r['confidence']['words']:
    assert np.abs(np.array(r['confidence']['words']) - np.exp(ref['log_conf'])).max() <= 1e-9
  line = alignment.result_json(r)
  assert [w['word'] for w in line['words']] == r['text'].split() and all(set(w) == {'word', 'start', 'end', 'confidence'} for w in line['words'])
  a = al[0]
  assert a['error'] is None and (a['spans'] == al_plain[0]['spans']).all() and a['score'] == al_plain[0]['score']
  assert len(a['confidence']['words']) == len(a['text'].split()) and all(0.0 <= c <= 1.0 for c in a['confidence']['words'])
  # the command line
  audio = tmp_path / 'audio'
  audio.mkdir()
  shutil.copy(GOLDEN_FLAC, str(audio / '1089-134686-0037.flac'))
  shutil.copy(os.path.join(GOLDEN, '1089-134686.trans.txt'), str(audio / '1089-134686.trans.txt'))
  first = str(audio / '1089-134686-0037.flac')
  base = ['--train-dir', str(train), '--run-name', 'run', '--device', dev]
  run = lambda args: subprocess.run([sys.executable, os.path.join(ROOT, 'speecht-cli')] + args, capture_output=True, text=True,
                                    timeout=600, cwd=str(tmp_path))
  out = tmp_path / 'align.jsonl'
  got = run(['align'] + base + ['--confidence', '--output', str(out), first])
  assert got.returncode == 0, got.stderr
  rows = [l.split('\t') for l in got.stdout.splitlines()]
  assert [row[3] for row in rows] == a['text'].split() and all(len(row) == 5 and 0.0 <= float(row[4]) <= 1.0 for row in rows)
  rec, = [json.loads(l) for l in out.read_text().splitlines()]
  assert abs(rec['log_prob'] - a['confidence']['log_prob']) <= 1e-6 * abs(rec['log_prob'])
  assert [w['confidence'] for w in rec['words']] == [round(c, 6) for c in a['confidence']['words']]
  out2 = tmp_path / 'tr.jsonl'
  got2 = run(['transcribe'] + base + ['--confidence', '--output', str(out2), first])
  assert got2.returncode == 0, got2.stderr
  lines = got2.stdout.splitlines()
  assert lines[0] == '{}\t{}'.format(first, r['text'])
  assert [l.split('\t')[1:4] for l in lines[1:]] == [['-', '-', w] for w in r['text'].split()]
  rec2, = [json.loads(l) for l in out2.read_text().splitlines()]
  assert rec2['text'] == r['text'] and [w['word'] for w in rec2['words']] == r['text'].split()
  assert ('log_prob' in rec2) == (r['confidence'] is not None)


def test_segmented_and_masked_files_carry_confidences(dev, tmp_path):
  from speecht_amd.segmentation import SegmentOptions
  from speecht_amd.speech_model import Session
  from speecht_amd.transcription import transcribe_files
  model = _golden_model(tmp_path)
  opts = SegmentOptions()
  with Session(dev) as sess:
    model.init_session(sess)
    eng = model.engine
    plain = transcribe_files(eng, [GOLDEN_FLAC], batch_size=4, mask_padding=True, timestamps=True, segment=opts)
    timed = transcribe_files(eng, [GOLDEN_FLAC], batch_size=4, mask_padding=True, timestamps=True, segment=opts, confidence=True)
    bare = transcribe_files(eng, [GOLDEN_FLAC], batch_size=4, mask_padding=True, segment=opts, confidence=True)
    masked = transcribe_files(eng, [GOLDEN_FLAC], mask_padding=True, confidence=True)
    unmasked = transcribe_files(eng, [GOLDEN_FLAC], mask_padding=True)
  p, t, b = plain[0], timed[0], bare[0]
  assert t['error'] is None and len(t['segments']) == len(p['segments']) >= 1 and t['ids'] == p['ids'] == b['ids']
  for sp, st, sb in zip(p['segments'], t['segments'], b['segments']):
    assert st['ids'] == sp['ids'] == sb['ids'] and 'confidence' not in sp
    n = len(st['text'].split())
    if st['confidence'] is not None:
      assert len(st['confidence']['words']) == n and sb['confidence'] == st['confidence']
      assert [{k: w[k] for k in ('word', 'start', 'end')} for w in st['words']] == sp['words']
      assert [w['confidence'] for w in st['words']] == [w['confidence'] for w in sb['words']]
      assert all(set(w) == {'word', 'confidence'} and 0.0 <= w['confidence'] <= 1.0 for w in sb['words'])
  assert any(seg['confidence'] is not None for seg in t['segments'])
  assert masked[0]['ids'] == unmasked[0]['ids'] and len(masked[0]['confidence']['words']) == len(masked[0]['text'].split())
