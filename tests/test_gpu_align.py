"""Forced alignment on the GPU: st_ctc_align_f32 against the float64 oracle (tests/align_oracle.py) and, bit for bit, against its
host form (st_ctc_align_host -- the two share their arithmetic, csrc/ctc_align_core.h), through every states-per-lane dispatch
and up to 1 501 frames; `engine.align`, `transcribe(timestamps=True)` and `align_files` on top of it.

The accuracy condition and what was measured against it: tests/test_align_cpu.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import align_oracle as AO
from tests import workloads as WL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
GOLDEN_FLAC = os.path.join(GOLDEN, '1089-134686-0037.flac')
TINY_LM = os.path.join(GOLDEN, 'lm_tiny.arpa')
C_PITCH = 32

# (largest label, frames) per dispatch of the lattice: 1, 2, 3, 4, 5, 6, 8, 10, 12, 16 states per lane hold up to
# 31, 63, 95, 127, 159, 191, 255, 319, 383, 511 labels
DISPATCH = [(31, 70), (63, 140), (95, 300), (127, 501), (159, 501), (191, 640), (255, 800), (319, 1000), (383, 1200), (511, 1501)]


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def _csr(labels):
  lens = [len(l) for l in labels]
  offs = np.zeros(len(labels) + 1, dtype=np.int32)
  offs[1:] = np.cumsum(lens)
  return np.array([i for l in labels for i in l] + [0], dtype=np.int32), offs


def device_align(dev, logits, labels, seq_lens, max_label_len=None, want_states=True):
  """st_ctc_align_f32 on a dense [B, T, C] batch laid out as padded NWC (halo 0, c_pitch 32)
  -> (spans list, states [B, T], score [B], status [B])."""
  from speecht_amd import _lib
  from speecht_amd._lib import Tensor3
  lib = _lib.load()
  B, T, C = logits.shape
  ids, offs = _csr(labels)
  N = int(offs[-1])
  max_len = max([len(l) for l in labels] + [0]) if max_label_len is None else max_label_len
  x = torch.full((B, T, C_PITCH), 1e30, dtype=torch.float32, device=dev)      # the pitch columns must never be read
  x[:, :, :C] = torch.as_tensor(logits, dtype=torch.float32)
  to = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
  d_ids, d_offs, d_lens = to(ids), to(offs), to(np.asarray(seq_lens, dtype=np.int32))
  spans = torch.full((N + 1, 2), -7, dtype=torch.int32, device=dev)
  states = torch.full((B, T), -7, dtype=torch.int32, device=dev)
  score = torch.zeros(B, dtype=torch.float32, device=dev)
  status = torch.full((B,), -7, dtype=torch.int32, device=dev)
  need = lib.st_ctc_align_ws(B, T, max_len)
  ws = torch.empty(need // 4 + 4, dtype=torch.int32, device=dev)
  P = lambda t: ctypes.c_void_p(t.data_ptr())
  desc = Tensor3(x.data_ptr(), B, T, C, 0, T, C_PITCH)
  _lib.call('st_ctc_align_f32', ctypes.byref(desc), P(d_ids), P(d_offs), P(d_lens), max_len, P(spans),
            P(states) if want_states else None, P(score), P(status), P(ws), need,
            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
  torch.cuda.synchronize()
  spans = spans.cpu().numpy()
  assert (spans[-1] == -7).all()                        # nothing written past the last label
  return [spans[offs[b]:offs[b + 1]] for b in range(B)], states.cpu().numpy(), score.cpu().numpy(), status.cpu().numpy()


def dispatch_batch(rng, l_max, l_lo, frames, planted):
  """Five utterances of one dispatch: the longest label it holds, the shortest that needs it, a short one, an empty one and
  one that does not fit its frames; ragged lengths."""
  C = 29
  xs, labs, paths = [], [], []
  for L, T in ((l_max, frames), (l_lo, int(rng.integers(frames // 2, frames))), (int(rng.integers(1, 12)), int(rng.integers(20, frames))),
               (0, int(rng.integers(0, 30)))):
    lab = AO.random_labels(rng, L, C, repeat_prob=0.15)
    T = max(T, AO.min_frames(lab) + int(rng.integers(0, 3)))
    if T > frames:                                        # too many repeats for this frame count: thin them out
      lab = AO.random_labels(rng, L, C, repeat_prob=0.0)
      T = max(min(T, frames), AO.min_frames(lab))
    assert AO.min_frames(lab) <= T <= frames
    if planted and T > 0:
      x, path = AO.planted_logits(rng, lab, T, C)
      paths.append([u // 2 if u & 1 else -1 for u in path])
    else:
      x = AO.random_logits(rng, T, C, scale=float(rng.choice([0.05, 1.0, 4.0])))
      paths.append(None)
    xs.append(x)
    labs.append(lab)
  lab = AO.random_labels(rng, min(l_max, 40), C, repeat_prob=0.5)       # does not fit: one frame short
  xs.append(AO.random_logits(rng, AO.min_frames(lab) - 1, C))
  labs.append(lab)
  paths.append(None)
  return xs, labs, paths


def check_utterance(x, lab, spans, states, score, status, frames):
  T = x.shape[0]
  ref = AO.align64(x, lab)
  assert (states[T:frames] == -2).all()
  if ref is None:
    assert status != 0 and score == -np.inf and (spans == -1).all() and (states[:T] == -2).all()
    return ref, (0.0, 0.0)
  assert status == 0
  st = states[:T]
  assert AO.is_valid_alignment(st, lab)
  assert (spans == AO.spans_from_states(st, len(lab))).all()
  r = AO.accuracy_ratios(x, lab, st, float(score), ref[2])
  assert r[0] <= 1.0 and r[1] <= 1.0, r
  return ref, r


@pytest.mark.parametrize('planted', [False, True], ids=['random', 'planted'])
def test_kernel_against_oracle_and_host_form(dev, planted):
  from tests.test_align_cpu import host_align
  rng = np.random.default_rng(40 + int(planted))
  worst = [0.0, 0.0]
  l_lo = 0
  for l_max, frames in DISPATCH:
    xs, labs, paths = dispatch_batch(rng, l_max, l_lo + 1 if l_lo else 1, frames, planted)
    l_lo = l_max
    logits, lens = AO.pad_batch(xs, frames)
    spans, states, score, status = device_align(dev, logits, labs, lens)
    for b, (x, lab, path) in enumerate(zip(xs, labs, paths)):
      ref, r = check_utterance(x, lab, spans[b], states[b], score[b], status[b], frames)
      worst = [max(worst[0], r[0]), max(worst[1], r[1])]
      if path is not None:
        assert list(ref[0]) == path                               # first: the oracle finds the planted path
        assert list(states[b, :len(path)]) == path
    assert status.tolist() == [0, 0, 0, 0, 1]
    # the host form: identical, bit for bit
    h_spans, h_states, h_score, h_status = host_align(logits, labs, lens)
    assert (h_status == status).all() and (h_states == states).all()
    assert all((a == b).all() for a, b in zip(h_spans, spans))
    assert (h_score.view(np.int32) == score.view(np.int32)).all()
    # states may be left out; a second call gives the same bits
    spans2, _, score2, status2 = device_align(dev, logits, labs, lens, want_states=False)
    assert all((a == b).all() for a, b in zip(spans2, spans)) and (score2.view(np.int32) == score.view(np.int32)).all()
    assert (status2 == status).all()
  print('kernel, {} cases: largest ratio to the bound: path {:.3g}, score {:.3g}'.format('planted' if planted else 'random', *worst))


def test_one_bad_utterance_leaves_its_neighbours_alone(dev):
  rng = np.random.default_rng(9)
  C = 29
  labs = [AO.random_labels(rng, 40, C, 0.1), AO.random_labels(rng, 30, C), AO.random_labels(rng, 10, C), []]
  xs = [AO.random_logits(rng, 80, C), AO.random_logits(rng, 25, C), AO.random_logits(rng, 60, C), AO.random_logits(rng, 0, C)]
  logits, lens = AO.pad_batch(xs)
  spans, states, score, status = device_align(dev, logits, labs, lens)
  assert status.tolist() == [0, 1, 0, 0] and (spans[1] == -1).all() and score[1] == -np.inf and score[3] == 0.0
  assert (states[1] == -2).all() and (states[3] == -2).all()
  for b in (0, 2):
    s1, st1, sc1, stat1 = device_align(dev, logits[b:b + 1], [labs[b]], lens[b:b + 1], max_label_len=40)
    assert (s1[0] == spans[b]).all() and (st1[0] == states[b]).all() and sc1[0] == score[b] and stat1[0] == 0
  # lengths outside 0 .. frames and a label beyond the dispatch (max_label_len 12 holds 31) are refused per utterance
  lens_bad = lens.copy()
  lens_bad[2] = 81
  _, st, sc, stat = device_align(dev, logits, labs, lens_bad, max_label_len=12)
  assert stat.tolist() == [1, 1, 1, 0] and (st[:3] == -2).all()


def test_run_to_run(dev):
  rng = np.random.default_rng(10)
  C, B, T = 29, 16, 501
  labs = [AO.random_labels(rng, int(rng.integers(100, 151)), C, 0.1) for _ in range(B)]
  logits = np.stack([AO.random_logits(rng, T, C, 1.0) for _ in range(B)])
  lens = rng.integers(400, T + 1, B).astype(np.int32)
  a = device_align(dev, logits, labs, lens)
  b = device_align(dev, logits, labs, lens)
  assert (a[1] == b[1]).all() and (a[2].view(np.int32) == b[2].view(np.int32)).all() and (a[3] == b[3]).all()
  assert all((x == y).all() for x, y in zip(a[0], b[0])) and (a[3] == 0).all()


def _greedy_runs(classes, blank):
  """(class, first frame, end frame) of each output character of the greedy decoder (merge_repeated=True)."""
  runs, prev = [], None
  for t, c in enumerate(classes):
    if c != blank:
      if c != prev:
        runs.append([int(c), t, t + 1])
      else:
        runs[-1][2] = t + 1
    prev = c
  return runs


def test_engine_align_follows_the_greedy_path(dev):
  from speecht_amd.engine import Wav2LetterEngine
  layers = WL.w2l_layers(16, width=40, fc=72)
  params = WL.xavier_params(layers, seed=21, bias_range=0.3)
  params[-1] = (params[-1][0] * 100.0, params[-1][1] * 0.0)        # random weights whose greedy transcripts have 3 to 9 characters
  lengths = [260, 201, 124, 77]
  feats = [WL.synthetic_features(300 + i, t, 16).astype(np.float32) for i, t in enumerate(lengths)]
  x = np.zeros((len(feats), max(lengths), 16), dtype=np.float32)
  for b, f in enumerate(feats):
    x[b, :f.shape[0]] = f
  eng = Wav2LetterEngine(layers, device=dev)
  eng.set_weights(params)
  eng.load_batch(x, lengths)
  eng.forward()
  ids, _ = eng.greedy_decode()
  assert any(len(s) > 3 for s in ids)
  spans, score, status, states = eng.align(ids, return_states=True)
  logits = eng.logits_time_major().cpu().numpy().transpose(1, 0, 2)
  T_out = logits.shape[1]
  assert states.shape == (len(ids), T_out) and score.shape == (len(ids), 1) and (status == 0).all()
  for b, lab in enumerate(ids):
    Tb = lengths[b] // 2
    st = states[b, :Tb]
    assert (states[b, Tb:] == -2).all()
    assert AO.is_valid_alignment(st, lab)
    # the path's label sequence collapses to the ids
    classes = [lab[s] if s >= 0 else 28 for s in st]
    assert AO.states_from_classes(classes, 28)[1] == list(lab)
    assert [lab[k] for k in sorted({int(s) for s in st if s >= 0})] == list(lab)
    assert (spans[b] == AO.spans_from_states(st, len(lab))).all()
    runs = _greedy_runs(np.argmax(logits[b, :Tb], axis=1), 28)
    assert [r[0] for r in runs] == list(lab)
    for k, (a, e) in enumerate(spans[b]):
      lo = runs[k - 1][2] if k else 0
      hi = runs[k + 1][1] if k + 1 < len(runs) else Tb
      assert lo <= a < e <= hi, (b, k)
    ref = AO.align64(logits[b, :Tb], lab)
    r = AO.accuracy_ratios(logits[b, :Tb], lab, st, float(score[b, 0]), ref[2])
    assert r[0] <= 1.0 and r[1] <= 1.0
  # refused on the host: wrong batch, ids outside the classes, too long
  with pytest.raises(ValueError):
    eng.align(ids[:2])
  with pytest.raises(ValueError):
    eng.align([[28]] + ids[1:])
  with pytest.raises(ValueError):
    eng.align([[1] * 512] + ids[1:])
  # a transcript that does not fit is a status, and the others are aligned as before
  spans2, score2, status2 = eng.align([[1, 2] * 40] + ids[1:3] + [[3] * 39])
  assert status2.tolist() == [0, 0, 0, 1] and (spans2[3] == -1).all() and score2[3, 0] == -np.inf
  assert all((spans2[b] == spans[b]).all() for b in (1, 2)) and (score2[1:3] == score[1:3]).all()


def test_transcribe_with_timestamps_keeps_the_ids(dev):
  from speecht_amd.alignment import word_spans
  from speecht_amd.engine import Wav2LetterEngine
  from speecht_amd.inference import align, transcribe
  layers = WL.w2l_layers(16, width=40, fc=72)
  params = WL.xavier_params(layers, seed=21, bias_range=0.3)
  params[-1] = (params[-1][0] * 12.0, params[-1][1] * 4.0)
  rng = np.random.default_rng(8)
  lengths = rng.integers(60, 260, 9).tolist()
  feats = [WL.synthetic_features(300 + i, t, 16).astype(np.float32) for i, t in enumerate(lengths)]
  eng = Wav2LetterEngine(layers, device=dev)
  eng.set_weights(params)
  for decode in ({}, dict(beam_width=16), dict(language_model=TINY_LM, beam_width=32, lm_options=dict(lm_weight=2.0))):
    for bs in (1, 4):
      ids, texts = transcribe(eng, feats, batch_size=bs, **decode)
      ids_t, texts_t, spans = transcribe(eng, feats, batch_size=bs, timestamps=True, **decode)
      assert ids_t == ids and texts_t == texts, (decode, bs)
      assert any(len(s) > 0 for s in ids)
      for i, (lab, sp) in enumerate(zip(ids, spans)):
        assert sp.shape == (len(lab), 2) and sp.dtype == np.int32
        if len(lab):
          assert (sp[:, 0] < sp[:, 1]).all() and (sp[1:, 0] >= sp[:-1, 1]).all()
          assert sp[0, 0] >= 0 and sp[-1, 1] <= lengths[i] // 2
        words = word_spans(lab, sp)
        assert [w for w, _, _ in words] == texts[i].split()
    if not decode:
      # inference.align on the decoded ids: the spans transcribe returned
      sp_a, sc_a, st_a = align(eng, feats, ids, batch_size=4)
      assert all((a == b).all() for a, b in zip(sp_a, spans)) and all(s == 0 for s in st_a) and all(np.isfinite(sc_a))
  assert transcribe(eng, [], timestamps=True) == ([], [], [])


def test_align_files_on_the_golden_flac(dev, tmp_path):
  from speecht_amd import alignment
  from speecht_amd.speech_input import SingleInputLoader
  from speecht_amd.speech_model import Session, Wav2LetterModel
  loader = SingleInputLoader(128)
  model = Wav2LetterModel(loader, 128, 29)
  model.add_training_ops()
  model.add_decoding_ops()
  model.finalize(str(tmp_path / 'log'), 'r', 'record')
  model.init_seed = 1234
  other = str(tmp_path / 'untranscribed.flac')
  with open(GOLDEN_FLAC, 'rb') as src, open(other, 'wb') as dst:
    dst.write(src.read())
  paths = [GOLDEN_FLAC, other]
  transcripts = alignment.find_transcripts(paths)
  text = alignment.read_transcripts(os.path.join(GOLDEN, '1089-134686.trans.txt'))['1089-134686-0037']
  assert transcripts == {GOLDEN_FLAC: text, other: None}
  with Session(dev) as sess:
    model.init_session(sess)
    timings = {}
    res = alignment.align_files(model.engine, paths, transcripts, timings=timings)
    again = alignment.align_files(model.engine, paths, transcripts)
  assert [r['path'] for r in res] == paths and set(timings) == {'decode_host', 'features', 'align'}
  assert 'no transcript' in res[1]['error'] and res[1]['spans'] is None
  r = res[0]
  assert r['error'] is None and r['text'] == text.lower() and r['sample_rate'] == 22050
  assert r['spans'].shape == (len(r['ids']), 2) and np.isfinite(r['score']) and r['score'] < 0.0
  assert (again[0]['spans'] == r['spans']).all() and again[0]['score'] == r['score']
  words = alignment.timed_words(r['ids'], r['spans'], r['sample_rate'], r['seconds'])
  assert [w['word'] for w in words] == text.lower().split()               # the words, in transcript order
  prev = 0.0
  for w in words:
    assert 0.0 <= prev <= w['start'] <= w['end'] <= r['seconds']          # monotone, not overlapping, inside the file
    prev = w['end']
  assert words[-1]['end'] > words[0]['start']
  line = alignment.result_json(r, chars=True)
  assert set(line) == {'path', 'seconds', 'text', 'score', 'score_per_frame', 'words', 'chars'}
  assert len(line['chars']) == len(r['ids']) and line['words'] == words
  assert abs(line['score_per_frame'] - r['score'] / r['frames']) < 1e-12


def test_cli_align_and_transcribe_timestamps_end_to_end(dev, tmp_path):
  import json
  import shutil
  import subprocess
  import sys
  from speecht_amd.speech_input import SingleInputLoader
  from speecht_amd.speech_model import Session, Wav2LetterModel
  loader = SingleInputLoader(128)
  model = Wav2LetterModel(loader, 128, 29)
  model.add_training_ops()
  model.add_decoding_ops()
  model.finalize(str(tmp_path / 'log'), 'r', 'record')
  model.init_seed = 1234
  train = tmp_path / 'train'
  (train / 'run').mkdir(parents=True)
  with Session(dev) as sess:
    model.init_session(sess)
    model.saver.save(sess, str(train / 'run' / 'speechT'), global_step=model.global_step)
  audio = tmp_path / 'audio'
  audio.mkdir()
  shutil.copy(GOLDEN_FLAC, str(audio / '1089-134686-0037.flac'))
  shutil.copy(os.path.join(GOLDEN, '1089-134686.trans.txt'), str(audio / '1089-134686.trans.txt'))
  shutil.copy(GOLDEN_FLAC, str(audio / 'zz-untranscribed.flac'))
  cwd = tmp_path / 'cwd'
  cwd.mkdir()
  base = ['--train-dir', str(train), '--run-name', 'run', '--device', dev]
  run = lambda args: subprocess.run([sys.executable, os.path.join(ROOT, 'speecht-cli')] + args, capture_output=True, text=True,
                                    timeout=600, cwd=str(cwd))
  out = tmp_path / 'align.jsonl'
  r = run(['align'] + base + ['--chars', '--output', str(out), str(audio)])
  assert r.returncode == 1 and 'zz-untranscribed.flac: no transcript' in r.stderr, r.stderr     # one file fails, the other is aligned
  first = str(audio / '1089-134686-0037.flac')
  rows = [l.split('\t') for l in r.stdout.splitlines()]
  from speecht_amd.alignment import read_transcripts
  text = read_transcripts(os.path.join(GOLDEN, '1089-134686.trans.txt'))['1089-134686-0037'].lower()
  assert [row[0] for row in rows] == [first] * len(text.split()) and [row[3] for row in rows] == text.split()
  times = [(float(row[1]), float(row[2])) for row in rows]
  assert all(a <= b for a, b in times) and all(times[k][1] <= times[k + 1][0] + 1e-9 for k in range(len(times) - 1))
  rec, = [json.loads(l) for l in out.read_text().splitlines()]
  assert rec['path'] == first and rec['text'] == text and [w['word'] for w in rec['words']] == text.split()
  assert len(rec['chars']) == len(text) and rec['score'] < 0 and times[-1][1] <= rec['seconds'] + 1e-3
  assert sorted(os.listdir(str(cwd))) == []
  # the transcript file given by name
  r2 = run(['align'] + base + ['--transcripts', str(audio / '1089-134686.trans.txt'), first])
  assert r2.returncode == 0 and r2.stdout == r.stdout, r2.stderr
  # transcribe --timestamps: the transcript line as without it, then the words of that text
  plain = run(['transcribe'] + base + [first])
  out2 = tmp_path / 'tr.jsonl'
  timed = run(['transcribe'] + base + ['--timestamps', '--output', str(out2), first])
  assert plain.returncode == 0 and timed.returncode == 0, timed.stderr
  lines = timed.stdout.splitlines()
  assert lines[0] == plain.stdout.splitlines()[0]
  decoded = lines[0].split('\t', 1)[1]
  assert [l.split('\t')[3] for l in lines[1:]] == decoded.split()
  rec2, = [json.loads(l) for l in out2.read_text().splitlines()]
  assert rec2['text'] == decoded and [w['word'] for w in rec2['words']] == decoded.split()
