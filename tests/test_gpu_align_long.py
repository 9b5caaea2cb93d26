"""Tiled forced alignment on the GPU: st_ctc_align_long_f32 against its host form (st_ctc_align_long_host, plain loops over the
whole lattice with the shared arithmetic of csrc/ctc_align_core.h) bit for bit -- spans, the score's bits, status -- at the
edges of the state blocks and of the frame blocks, on the forced diagonal that crosses block edges two states per frame, on
ties, on -inf logits; against st_ctc_align_f32 where that kernel can run, against the float64 oracle, and end to end through
`align_files(segment=...)` and `speecht-cli align --segment`.  No case is larger than 3 000 frames x 2 000 labels."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

from tests import align_oracle as AO
from tests.align_long_util import (device_align_long, edge_labels, host_align_long, same_result, states_from_spans,
                                   workspace_bytes)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
GOLDEN_FLAC = os.path.join(GOLDEN, '1089-134686-0037.flac')
C = 29


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def _blocks():
  from speecht_amd import engine_decode as ED
  return ED.ALIGN_LONG_STATE_BLOCK, ED.ALIGN_LONG_FRAME_BLOCK


def _both(dev, x, lab, **kw):
  """Device and host form on the same input; they must agree bit for bit.  -> the device's (spans, score, status)."""
  d = device_align_long(dev, x, lab, **kw)
  h = host_align_long(x, lab)
  assert same_result(d, h), (len(lab), x.shape, d[1], h[1], d[2], h[2], int((d[0] != h[0]).sum()))
  return d


def _edge_lengths():
  S, _ = 896, 64
  return [(S - 2) // 2, S // 2, (2 * S - 2) // 2, (2 * S) // 2, (3 * S) // 2, 0, 1, 511, 512]


@pytest.mark.parametrize('L', _edge_lengths())
def test_state_block_and_frame_block_edges(dev, L):
  """Labels whose 2L+1 states end one short of, or one past, a state-block edge, with repeats on the ids whose states straddle
  the edges, at frame counts on the fit rule's edge and around a multiple of the frame block."""
  S, F = _blocks()
  assert 2 * L + 1 in (S - 1, S + 1, 2 * S - 1, 2 * S + 1, 3 * S + 1) or L in (0, 1, 511, 512)
  rng = np.random.default_rng(100 + L)
  lab = edge_labels(rng, L, C, edges=(S, 2 * S))
  for e in (S, 2 * S):
    if e // 2 + 1 < L:
      assert lab[e // 2 - 1] == lab[e // 2] == lab[e // 2 + 1]
  need = AO.min_frames(lab)
  m = (need // F + 2) * F
  for T in (max(need, 1), need + 1, m, m - 1, m + 1):
    x = AO.random_logits(rng, T, C, scale=float(rng.choice([0.05, 1.0, 3.0])))
    spans, score, status = _both(dev, x, lab)
    assert status == 0 and np.isfinite(score)
    assert AO.is_valid_alignment(states_from_spans(spans, T), lab)


def test_forced_diagonal_across_two_block_edges(dev):
  """T = L with neighbouring ids always different: the only path advances two states per frame, across the state-block edges
  at 896, 1 792, ... inside frame blocks -- what the halo of 2 * 64 states exists for."""
  L = 2000
  lab = [(5 * k) % 28 for k in range(L)]
  rng = np.random.default_rng(5)
  x = AO.random_logits(rng, L, C)
  spans, score, status = _both(dev, x, lab)
  assert status == 0
  assert (spans == np.stack([np.arange(L), np.arange(L) + 1], axis=1)).all()
  ly = AO.log_softmax64(x)
  assert abs(score - ly[np.arange(L), lab].sum()) <= 1e-9 * abs(score)
  spans, score, status = _both(dev, AO.random_logits(rng, L + 1, C), lab)
  assert status == 0 and AO.is_valid_alignment(states_from_spans(spans, L + 1), lab)


def test_ties(dev):
  """All-zero logits (every comparison is an exact tie: the tie rule alone decides) and logits rounded to integers."""
  rng = np.random.default_rng(6)
  L, T = 1000, 1500
  lab = edge_labels(rng, L, C, repeat_prob=0.1)
  assert AO.min_frames(lab) <= T
  zero = np.zeros((T, C), dtype=np.float32)
  spans, score, status = _both(dev, zero, lab)
  assert status == 0 and (spans == AO.align64(zero, lab)[1]).all()
  spans, score, status = _both(dev, np.round(AO.random_logits(rng, T, C, scale=1.5)), lab)
  assert status == 0 and AO.is_valid_alignment(states_from_spans(spans, T), lab)


def test_infinite_logits_and_a_label_that_does_not_fit(dev):
  rng = np.random.default_rng(7)
  L, T = 600, 1000
  lab = edge_labels(rng, L, C, repeat_prob=0.1)
  x = AO.random_logits(rng, T, C)
  x[rng.random((T, C)) < 0.1] = -np.inf
  x[:, C - 1] = np.where(np.isinf(x[:, C - 1]), 0.0, x[:, C - 1])          # (the blank stays: a path of finite score exists)
  x[np.arange(T), rng.integers(0, C - 1, T)] = 1.0
  spans, score, status = _both(dev, x, lab)
  assert status == 0
  need = AO.min_frames(lab)
  spans, score, status = _both(dev, AO.random_logits(rng, need - 1, C), lab)
  assert status == 1 and score == -np.inf and (spans == -1).all()
  spans, score, status = _both(dev, AO.random_logits(rng, need, C), lab)
  assert status == 0 and np.isfinite(score)


@pytest.mark.parametrize('L,T', [(20, 130), (511, 1100)])
def test_equals_the_one_wave_kernel_where_it_runs(dev, L, T):
  """Labels st_ctc_align_f32 takes (1 and 16 states per lane), B = 1, the same logits: the same spans, the same score as a float."""
  from tests.test_gpu_align import device_align
  rng = np.random.default_rng(8 + L)
  lab = AO.random_labels(rng, L, C)
  T = max(T, AO.min_frames(lab))
  for x in (AO.random_logits(rng, T, C), AO.planted_logits(rng, lab, T, C)[0], np.zeros((T, C), dtype=np.float32)):
    spans, score, status = _both(dev, x, lab)
    s1, _, sc1, st1 = device_align(dev, x[None], [lab], [T])
    assert status == 0 and st1[0] == 0 and (spans == s1[0]).all() and np.float32(score) == sc1[0]


def test_workspace_hygiene(dev):
  """A workspace full of 0xFF bytes, then a different, shorter label in the same workspace."""
  from speecht_amd import _lib
  rng = np.random.default_rng(9)
  L, T = 1000, 1300
  lab = edge_labels(rng, L, C, repeat_prob=0.1)
  x = AO.random_logits(rng, T, C)
  ws = torch.full((_lib.load().st_ctc_align_long_ws(T, L) // 4 + 4,), -1, dtype=torch.int32, device=dev)
  _both(dev, x, lab, workspace=ws)
  short = AO.random_labels(rng, 300, C)
  _both(dev, x[:777], short, workspace=ws)
  _both(dev, x, lab, workspace=ws)


def test_against_the_oracle(dev):
  rng = np.random.default_rng(10)
  L, T = 1400, 3000
  lab = edge_labels(rng, L, C)
  x = AO.random_logits(rng, T, C)
  spans, score, status = _both(dev, x, lab)
  ref = AO.align64(x, lab)
  states = states_from_spans(spans, T)
  assert status == 0 and AO.is_valid_alignment(states, lab)
  r = AO.accuracy_ratios(x, lab, states, score, ref[2])
  print('T = 3000, L = 1400: ratios to the accuracy bounds: path {:.3g}, score {:.3g}'.format(*r))
  assert r[0] <= 1.0 and r[1] <= 1.0
  xp, path = AO.planted_logits(rng, lab, T, C)
  spans, score, status = _both(dev, xp, lab)
  assert (spans == AO.align64(xp, lab)[1]).all()


def test_engine_align_long_checks_its_arguments(dev):
  from tests import workloads as WL
  from speecht_amd.engine import Wav2LetterEngine
  eng = Wav2LetterEngine(WL.w2l_layers(16, width=40, fc=72), device=dev)
  rng = np.random.default_rng(11)
  C_eng = eng.num_classes
  lab = AO.random_labels(rng, 700, C_eng)
  x = AO.random_logits(rng, 1000, C_eng)
  spans, score, status = eng.align_long(torch.as_tensor(x).to(dev), lab)
  assert same_result((spans, score, status), host_align_long(x, lab)) and spans.dtype == np.int32
  padded = torch.full((1000, C_eng + 3), 1e30, dtype=torch.float32, device=dev)
  padded[:, :C_eng] = torch.as_tensor(x).to(dev)
  assert same_result(eng.align_long(padded, lab), (spans, score, status))
  with pytest.raises(ValueError, match='label ids'):
    eng.align_long(torch.as_tensor(x).to(dev), [C_eng - 1])
  with pytest.raises(ValueError, match=str(workspace_bytes(1000, 700))):
    eng.align_long(torch.as_tensor(x).to(dev), lab, max_workspace_bytes=1 << 16)
  with pytest.raises(ValueError):
    eng.align_long(x, lab)


def _write_wav(path, samples, rate):
  with wave.open(path, 'wb') as w:
    w.setnchannels(1)
    w.setsampwidth(2)
    w.setframerate(rate)
    w.writeframes(np.round(np.clip(samples, -1, 1) * 32767).astype('<i2').tobytes())


def test_long_recording_end_to_end(dev, tmp_path):
  """The golden FLAC twelve times with half a second of zeros between the copies and its transcript twelve times: more than
  511 characters, aligned as one transcript against the concatenated frames of the segments."""
  from speecht_amd import alignment, inference, segmentation, transcription
  from speecht_amd.speech_input import SingleInputLoader
  from speecht_amd.speech_model import Session, Wav2LetterModel
  samples, rate = transcription.load_native(GOLDEN_FLAC)
  gap = np.zeros(rate // 2, dtype=np.float32)
  audio = tmp_path / 'audio'
  audio.mkdir()
  path = str(audio / 'long.wav')
  _write_wav(path, np.concatenate(sum([[samples, gap] for _ in range(12)], [])[:-1]), rate)
  text = alignment.read_transcripts(os.path.join(GOLDEN, '1089-134686.trans.txt'))['1089-134686-0037']
  long_text = ' '.join([text] * 12)
  assert len(long_text) > 511
  (audio / 'long.trans.txt').write_text('long ' + long_text + '\n')
  model = Wav2LetterModel(SingleInputLoader(128), 128, 29)
  model.add_training_ops()
  model.add_decoding_ops()
  model.finalize(str(tmp_path / 'log'), 'r', 'record')
  model.init_seed = 1234
  train = tmp_path / 'train'
  (train / 'run').mkdir(parents=True)
  options = segmentation.SegmentOptions()
  with Session(dev) as sess:
    model.init_session(sess)
    model.saver.save(sess, str(train / 'run' / 'speechT'), global_step=model.global_step)
    transcripts = alignment.find_transcripts([path])
    r, = alignment.align_files(model.engine, [path], transcripts, segment=options, batch_size=4, mask_padding=True)
    again, = alignment.align_files(model.engine, [path], transcripts, segment=options, batch_size=4, mask_padding=True)
    short, = alignment.align_files(model.engine, [path], transcripts)
    # the same segments through the layers below: the logits align_files gathered, and the host form on them
    data, file_rate = transcription.load_native(path)
    table, gathered, offsets = segmentation.segment_audio([data], [file_rate], options, dev)
    feats = transcription.device_features_on_device(gathered, offsets, [file_rate] * len(table))
    spans, score, status, frames, logits = inference.align_long(model.engine, [f for f in feats if f is not None], r['ids'],
                                                                batch_size=4, mask_padding=True, return_logits=True)
    host = host_align_long(logits.cpu().numpy(), r['ids'])
  assert 'too long to align (max 511)' in short['error'] and short['spans'] is None
  assert r['error'] is None and r['text'] == long_text.lower() and len(r['segments']) >= 12
  assert r['frames'] == sum(r['segment_frames']) == logits.shape[0] and list(frames) == [n for n in r['segment_frames'] if n]
  assert status == 0 and same_result((spans, score, status), host)
  assert (r['spans'] == host[0]).all() and r['score'] == host[1]
  assert (again['spans'] == r['spans']).all() and again['score'] == r['score'] and again['segments'] == r['segments']
  words = alignment.timed_words(r['ids'], r['spans'], r['sample_rate'], r['seconds'], concat=alignment.concat_of(r))
  assert [w['word'] for w in words] == long_text.lower().split()
  prev = 0.0
  for w in words:
    assert 0.0 <= prev <= w['start'] <= w['end'] <= r['seconds'], w
    prev = w['end']
  line = alignment.result_json(r)
  assert line['words'] == words and len(line['segments']) == len(r['segments'])
  # the CLI: the same words and times, and no directory
  cwd = tmp_path / 'cwd'
  cwd.mkdir()
  out = tmp_path / 'long.jsonl'
  base = ['--train-dir', str(train), '--run-name', 'run', '--device', dev]
  run = lambda args: subprocess.run([sys.executable, os.path.join(ROOT, 'speecht-cli'), 'align'] + base + args, capture_output=True,
                                    text=True, timeout=600, cwd=str(cwd))
  c = run(['--segment', '--batch-size', '4', '--mask-padding', '--output', str(out), str(audio)])
  assert c.returncode == 0, c.stderr
  rows = [l.split('\t') for l in c.stdout.splitlines()]
  assert [row[3] for row in rows] == [w['word'] for w in words]
  assert [(float(row[1]), float(row[2])) for row in rows] == [(float('{:.3f}'.format(w['start'])), float('{:.3f}'.format(w['end']))) for w in words]
  rec, = [json.loads(l) for l in out.read_text().splitlines()]
  assert rec['words'] == words and rec['score'] == r['score']
  assert sorted(os.listdir(str(cwd))) == []
