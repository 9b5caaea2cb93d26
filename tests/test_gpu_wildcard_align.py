"""The wildcard label and the per-label fit on the GPU: st_ctc_align_wild_f32 and st_ctc_align_long_wild_f32 against their host
forms bit for bit (spans, states, the score's bits, status, the fit's bits -- they share csrc/ctc_align_core.h) and against the
float64 oracle (tests/wildcard_align_oracle.py) under the accuracy conditions of tests/test_gpu_align.py; through every
states-per-lane dispatch of the one-wave aligner, at the state-block and frame-block edges of the tiled one; against each other
and against the plain entry points; and end to end through `engine.align`, `align_files` and `speecht-cli align --segment`.
No case is larger than 3 000 frames x 1 400 labels."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import align_oracle as AO
from tests import wildcard_align_oracle as WO
from tests import wildcard_align_util as WU
from tests.align_long_util import device_align_long, edge_labels, states_from_spans
from tests.test_gpu_align import DISPATCH, device_align

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
GOLDEN_FLAC = os.path.join(GOLDEN, '1089-134686-0037.flac')
CLASSES = (29, 2, 31)


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def _same_batch(d, h):
  """Device and host results of the one-wave aligner agree bit for bit."""
  assert (d[3] == h[3]).all() and (d[1] == h[1]).all()
  assert (d[2].view(np.int32) == h[2].view(np.int32)).all()
  assert all((a == b).all() for a, b in zip(d[0], h[0]))
  for a, b in zip(d[4], h[4]):
    assert (np.isnan(a) == np.isnan(b)).all() and (WU.bits(a)[~np.isnan(a)] == WU.bits(b)[~np.isnan(b)]).all()


def _labels(rng, L, C):
  return AO.random_labels(rng, L, C, repeat_prob=0.15 if C > 2 else 1.0)


def wild_dispatch_batch(rng, l_max, l_lo, frames, C):
  """Seven utterances of one dispatch: a label inside it with every fifth id a wildcard; one with a wildcard first, on the fewest
  frames the fit rule takes; one with a wildcard last, on one frame more; a wildcard alone; one between equal ids; the longest
  label the dispatch holds, wildcards at both ends; and one that does not fit its frames -- one frame short once its wildcards
  count."""
  W = WO.wild_id(C)
  inside = int(rng.integers(l_lo, l_max)) if l_max > l_lo else l_max
  labs = [WU.with_wildcards(_labels(rng, inside, C), C, 'fifth'),
          WU.with_wildcards(_labels(rng, max(inside // 2, 1), C), C, 'first'),
          WU.with_wildcards(_labels(rng, max(inside // 2, 1), C), C, 'last'),
          [W], [0, W, 0],
          WU.with_wildcards(_labels(rng, l_max - 2, C), C, 'ends'),
          WU.with_wildcards(_labels(rng, min(l_max - 2, 40), C), C, 'ends')]
  need = [AO.min_frames(l) for l in labs]
  assert max(need) <= frames and max(len(l) for l in labs) == l_max
  Ts = [frames, need[1], need[2] + 1, int(rng.integers(1, 40)), int(rng.integers(3, 40)), max(need[5], frames - int(rng.integers(0, 9))),
        need[6] - 1]
  xs = [AO.random_logits(rng, t, C, scale=float(rng.choice([0.05, 1.0, 4.0]))) for t in Ts]
  return xs, labs


@pytest.mark.parametrize('k', range(len(DISPATCH)), ids=['labels{}'.format(d[0]) for d in DISPATCH])
def test_one_wave_kernel_against_host_form_and_oracle(dev, k):
  """One label length inside each states-per-lane class and the longest it holds (the last: 511); C in {29, 2, 31} by turns and
  all three at the first; wildcards first, last, alone, every fifth label, between equal ids; the fit rule's edge and one frame
  more; a refused utterance among the others."""
  l_max, frames = DISPATCH[k]
  l_lo = DISPATCH[k - 1][0] + 1 if k else 3
  worst = [0.0, 0.0]
  for C in (CLASSES if k == 0 else (CLASSES[k % 3],)):
    rng = np.random.default_rng(300 + 10 * k + C)
    bias = float(rng.choice([-1.0, -0.5, 0.0]))
    xs, labs = wild_dispatch_batch(rng, l_max, l_lo, frames, C)
    logits, lens = AO.pad_batch(xs, frames)
    d = WU.device_align_wild(dev, logits, labs, lens, bias)
    assert d[3].tolist() == [0, 0, 0, 0, 0, 0, 1]
    _same_batch(d, WU.host_align_wild(logits, labs, lens, bias))
    for b, (x, lab) in enumerate(zip(xs, labs)):
      r = WU.check_wild_utterance(x, lab, d[0][b], d[1][b], d[2][b], d[3][b], d[4][b], bias, frames)
      worst = [max(worst[0], r[0]), max(worst[1], r[1])]
    # states and the fit may be left out; a second call gives the same bits
    again = WU.device_align_wild(dev, logits, labs, lens, bias, want_states=False, want_fit=False)
    assert all((a == b).all() for a, b in zip(again[0], d[0])) and (again[2].view(np.int32) == d[2].view(np.int32)).all()
    assert (again[3] == d[3]).all() and all((f == 7.0).all() for f in again[4])
  print('{} labels: largest ratio to the bound: path {:.3g}, score {:.3g}'.format(l_max, *worst))


def test_planted_gap_on_the_device(dev):
  """The experiment of tests/test_wildcard_align_cpu.py as one batch of 40: the kernel gives what the host form gives there."""
  rng = np.random.default_rng(2024)
  cases = [WO.planted_gap_case(rng) for _ in range(40)]
  labs = [l1 + [29] + l2 for _, l1, l2, _, _ in cases]
  logits = np.stack([c[0] for c in cases])
  lens = [logits.shape[1]] * 40
  d = WU.device_align_wild(dev, logits, labs, lens, -1.0)
  _same_batch(d, WU.host_align_wild(logits, labs, lens, -1.0))
  exact = 0
  for (x, l1, l2, g0, g1), spans in zip(cases, d[0]):
    want = np.concatenate([AO.align64(x[:g0], l1)[1], AO.align64(x[g1:], l2)[1] + g1])
    off = int(np.abs(np.concatenate([spans[:len(l1)], spans[len(l1) + 1:]]) - want).max())
    assert off <= 2 and g0 - 3 <= spans[len(l1)][0] < spans[len(l1)][1] <= g1 + 3
    exact += off == 0
  assert exact >= 36


WILD_AT = [(447,), (448,), (895,), (896,), (446, 448), (894, 897), (400, 850), (0, 447, 999)]


@pytest.mark.parametrize('at', WILD_AT, ids=['-'.join(map(str, a)) for a in WILD_AT])
def test_tiled_kernel_at_the_block_edges(dev, at):
  """The labels of align_long_util.edge_labels (1 000 ids: 2 001 states in three state blocks, repeats across the edges) with
  wildcards on the labels whose states are 895 and 897 (around the blank state 896, the first state of the second block) and 1 791
  and 1 793, on both sides of an edge at once, and inside the 128-state halo below an edge (labels 400, 850: states 801, 1 701);
  frames on the fit rule's edge and around multiples of 64."""
  C, L = 29, 1000
  W = WO.wild_id(C)
  rng = np.random.default_rng(400 + sum(at))
  lab = edge_labels(rng, L, C, edges=(896, 1792))
  for k in at:
    lab[k] = W
  need = AO.min_frames(lab)
  m = (need // 64 + 2) * 64
  for T, bias in ((need, -1.0), (need + 1, -1.0), (m - 1, -0.5), (m, -1.0), (m + 1, 0.0)):
    x = AO.random_logits(rng, T, C, scale=float(rng.choice([0.05, 1.0, 3.0])))
    d = WU.device_align_long_wild(dev, x, lab, bias)
    h = WU.host_align_long_wild(x, lab, bias)
    assert WU.same_long(d, h), (at, T, d[1], h[1], d[2], h[2], int((d[0] != h[0]).sum()))
    assert d[2] == 0 and np.isfinite(d[1]) and AO.is_valid_alignment(states_from_spans(d[0], T), lab)
    WU.check_fit(x, lab, d[0], d[3], bias)
  x = AO.random_logits(rng, need - 1, C)
  d = WU.device_align_long_wild(dev, x, lab, -1.0)
  assert WU.same_long(d, WU.host_align_long_wild(x, lab, -1.0)) and d[2] == 1 and d[1] == -np.inf and (d[0] == -1).all()
  assert np.isnan(d[3]).all()


def test_tiled_kernel_against_the_oracle(dev):
  """3 000 frames x 1 400 labels, every twentieth a wildcard: the oracle's accuracy conditions; planted logits with stretches
  the transcript leaves out: the oracle's spans; and one label forced over 2 000 frames: its fit is one long serial sum."""
  rng = np.random.default_rng(410)
  C, L, T = 29, 1400, 3000
  W = WO.wild_id(C)
  lab = edge_labels(rng, L, C)
  for k in range(7, L, 20):
    lab[k] = W
  x = AO.random_logits(rng, T, C)
  d = WU.device_align_long_wild(dev, x, lab, -1.0)
  assert WU.same_long(d, WU.host_align_long_wild(x, lab, -1.0))
  r = WU.check_wild_utterance(x, lab, d[0], None, d[1], d[2], d[3], -1.0)
  print('T = 3000, L = 1400: ratios to the accuracy bounds: path {:.3g}, score {:.3g}'.format(*r))
  full = edge_labels(rng, L, C)
  xp, _ = AO.planted_logits(rng, full, T, C)
  cut = full[:300] + [W] + full[340:900] + [W] + full[910:]
  d = WU.device_align_long_wild(dev, xp, cut, -1.0)
  ref = WO.align_wild64(xp, cut, -1.0)
  assert d[2] == 0 and (d[0] == ref[1]).all()
  WU.check_fit(xp, cut, d[0], d[3], -1.0)
  assert d[0][300][1] - d[0][300][0] >= 40 and d[3][300] == -1.0 * (d[0][300][1] - d[0][300][0])
  forced = np.full((2000, C), -4.0, dtype=np.float32)
  forced[:, 3] = 4.0
  forced[1000:, 5] = rng.standard_normal(1000).astype(np.float32) + 4.0
  d = WU.device_align_long_wild(dev, forced, [3], -1.0)
  assert WU.same_long(d, WU.host_align_long_wild(forced, [3], -1.0)) and d[0].tolist() == [[0, 2000]]
  WU.check_fit(forced, [3], d[0], d[3], -1.0)
  assert d[3][0] < 0.0


@pytest.mark.parametrize('L,T', [(20, 130), (511, 1100)])
def test_both_aligners_agree_where_both_run(dev, L, T):
  C = 29
  rng = np.random.default_rng(420 + L)
  for where, bias in (('fifth', -1.0), ('ends', -0.5), ('first', 0.0)):
    lab = WU.with_wildcards(AO.random_labels(rng, L - 2, C), C, where)
    Tb = max(T, AO.min_frames(lab))
    for x in (AO.random_logits(rng, Tb, C), np.zeros((Tb, C), dtype=np.float32)):
      one = WU.device_align_wild(dev, x[None], [lab], [Tb], bias)
      tiled = WU.device_align_long_wild(dev, x, lab, bias)
      assert one[3][0] == 0 and tiled[2] == 0 and (one[0][0] == tiled[0]).all() and np.float32(tiled[1]) == one[2][0]
      assert (WU.bits(one[4][0]) == WU.bits(tiled[3])).all()


def test_without_a_wildcard_the_plain_entry_points(dev):
  """The same bits as st_ctc_align_f32 and st_ctc_align_long_f32, whatever the bias, and the fit of the plain path."""
  rng = np.random.default_rng(430)
  C, B, T = 29, 6, 300
  labs = [AO.random_labels(rng, int(rng.integers(0, 120)), C, 0.1) for _ in range(B - 1)] + [AO.random_labels(rng, 100, C, 0.0)]
  lens = [int(rng.integers(max(AO.min_frames(l), 1), T + 1)) for l in labs[:-1]] + [99]        # the last does not fit
  logits = np.stack([AO.random_logits(rng, T, C, 1.0) for _ in range(B)])
  plain = device_align(dev, logits, labs, lens)
  for bias in (0.0, -1.0):
    wild = WU.device_align_wild(dev, logits, labs, lens, bias)
    assert (wild[3] == plain[3]).all() and (wild[1] == plain[1]).all() and wild[3].tolist() == [0] * (B - 1) + [1]
    assert (wild[2].view(np.int32) == plain[2].view(np.int32)).all() and all((a == b).all() for a, b in zip(wild[0], plain[0]))
    for b in range(B - 1):
      WU.check_fit(logits[b, :lens[b]], labs[b], wild[0][b], wild[4][b], bias)
    assert np.isnan(wild[4][B - 1]).all()
  lab = edge_labels(rng, 1000, C)
  x = AO.random_logits(rng, 1500, C)
  p = device_align_long(dev, x, lab)
  w = WU.device_align_long_wild(dev, x, lab, -1.0)
  assert (w[0] == p[0]).all() and WU.bits([w[1]])[0] == WU.bits([p[1]])[0] and w[2] == p[2] == 0
  WU.check_fit(x, lab, w[0], w[3], -1.0)


def test_run_to_run(dev):
  rng = np.random.default_rng(440)
  C, B, T = 29, 16, 501
  labs = [WU.with_wildcards(AO.random_labels(rng, int(rng.integers(100, 151)), C, 0.1), C, 'fifth') for _ in range(B)]
  logits = np.stack([AO.random_logits(rng, T, C, 1.0) for _ in range(B)])
  lens = rng.integers(400, T + 1, B).astype(np.int32)
  a = WU.device_align_wild(dev, logits, labs, lens, -1.0)
  b = WU.device_align_wild(dev, logits, labs, lens, -1.0)
  _same_batch(a, b)
  assert (a[3] == 0).all()
  lab = WU.with_wildcards(edge_labels(rng, 1200, C), C, 'ends')
  x = AO.random_logits(rng, 2000, C)
  assert WU.same_long(WU.device_align_long_wild(dev, x, lab, -1.0), WU.device_align_long_wild(dev, x, lab, -1.0))


# ---- end to end -----------------------------------------------------------------------------------------------------------------

def test_engine_align_with_wildcards(dev):
  from tests import workloads as WL
  from speecht_amd import engine_decode as ED
  from speecht_amd.engine import Wav2LetterEngine
  layers = WL.w2l_layers(16, width=40, fc=72)
  params = WL.xavier_params(layers, seed=21, bias_range=0.3)
  params[-1] = (params[-1][0] * 100.0, params[-1][1] * 0.0)
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
  C = eng.num_classes
  plain = eng.align(ids, return_states=True)
  # the defaults take the old path and return the old tuple; fit=True alone adds the fits of the same path
  spans, score, status, fits = eng.align(ids, fit=True)
  assert len(plain) == 4 and all((a == b).all() for a, b in zip(spans, plain[0])) and (score == plain[1]).all()
  assert all((f == 0.0).all() for f in fits)                         # the greedy reading's own labels: every frame agrees
  # the middle of every transcript left out: a wildcard takes its place, the rest keeps its spans
  W = ED.WILDCARD
  cut = [l[:1] + [W] + l[-1:] if len(l) > 3 else list(l) for l in ids]
  spans_w, score_w, status_w, states_w, fits_w = eng.align(cut, return_states=True, wildcard_bias=-1.0)
  logits = eng.logits_time_major().cpu().numpy().transpose(1, 0, 2)
  for b, lab in enumerate(cut):
    Tb = lengths[b] // 2
    c_lab = [C if l == W else l for l in lab]
    host = WU.host_align_wild(logits[b:b + 1, :Tb], [c_lab], [Tb], -1.0)
    assert status_w[b] == 0 and (host[0][0] == spans_w[b]).all() and (host[1][0] == states_w[b, :Tb]).all()
    assert host[2][0] == score_w[b, 0] and (WU.bits(host[4][0]) == WU.bits(fits_w[b])).all()
    if W in lab:
      a, e = spans_w[b][1]
      # (how many frames it takes is the lattice's choice: these logits are nearly flat, and a frame misread costs less than 1 nat)
      assert fits_w[b][1] == -1.0 * (e - a) and e > a
  # refused on the host: a wildcard without the keyword arguments, two in a row, a bias above 0
  with pytest.raises(ValueError):
    eng.align(cut)
  with pytest.raises(ValueError, match='adjacent'):
    eng.align([[1, W, W, 2]] + ids[1:], fit=True)
  with pytest.raises(ValueError, match='wildcard_bias'):
    eng.align(ids, wildcard_bias=0.5)
  # align_long: the same arguments, the same answer on one utterance's frames
  b = int(np.argmax([len(l) for l in cut]))
  Tb = lengths[b] // 2
  sp, sc, st, ft = eng.align_long(torch.as_tensor(logits[b, :Tb].copy()).to(dev), cut[b], wildcard_bias=-1.0)
  assert st == 0 and (sp == spans_w[b]).all() and np.float32(sc) == score_w[b, 0] and (WU.bits(ft) == WU.bits(fits_w[b])).all()
  assert len(eng.align_long(torch.as_tensor(logits[b, :Tb].copy()).to(dev), ids[b])) == 3
  with pytest.raises(ValueError):
    eng.align_long(torch.as_tensor(logits[b, :Tb].copy()).to(dev), cut[b])


def _model(tmp_path):
  from speecht_amd.speech_input import SingleInputLoader
  from speecht_amd.speech_model import Wav2LetterModel
  model = Wav2LetterModel(SingleInputLoader(128), 128, 29)
  model.add_training_ops()
  model.add_decoding_ops()
  model.finalize(str(tmp_path / 'log'), 'r', 'record')
  model.init_seed = 1234
  return model


def test_align_files_and_the_cli_end_to_end(dev, tmp_path):
  """The golden FLAC with the first two words of its transcript replaced by `*`: `align_files(wildcard=..., fit=True)` with and
  without segment=, against the host form on the same logits, and `speecht-cli align --segment --wildcard --fit`."""
  from speecht_amd import alignment, inference, segmentation, transcription
  from speecht_amd.speech_model import Session
  text = alignment.read_transcripts(os.path.join(GOLDEN, '1089-134686.trans.txt'))['1089-134686-0037']
  star_text = ' '.join(['*'] + text.split()[2:])
  audio = tmp_path / 'audio'
  audio.mkdir()
  path = str(audio / '1089-134686-0037.flac')
  shutil.copy(GOLDEN_FLAC, path)
  (audio / 'x.trans.txt').write_text('1089-134686-0037 ' + star_text + '\n')
  model = _model(tmp_path)
  train = tmp_path / 'train'
  (train / 'run').mkdir(parents=True)
  options = segmentation.SegmentOptions()
  with Session(dev) as sess:
    model.init_session(sess)
    model.saver.save(sess, str(train / 'run' / 'speechT'), global_step=model.global_step)
    transcripts = alignment.find_transcripts([path])
    no_flag, = alignment.align_files(model.engine, [path], transcripts)
    r, = alignment.align_files(model.engine, [path], transcripts, wildcard='*', fit=True)
    again, = alignment.align_files(model.engine, [path], transcripts, wildcard='*', fit=True)
    ends, = alignment.align_files(model.engine, [path], {path: ' '.join(text.split()[2:])}, ends=True)
    seg, = alignment.align_files(model.engine, [path], transcripts, wildcard='*', fit=True, segment=options, mask_padding=True)
    # the logits below align_files(segment=...) and the host form on them
    data, rate = transcription.load_native(path)
    table, gathered, offsets = segmentation.segment_audio([data], [rate], options, dev)
    feats = transcription.device_features_on_device(gathered, offsets, [rate] * len(table))
    res = inference.align_long(model.engine, [f for f in feats if f is not None], seg['ids'], mask_padding=True, return_logits=True,
                               wildcard_bias=-1.0, fit=True)
    host = WU.host_align_long_wild(res[4].cpu().numpy(), [29 if i == alignment.WILDCARD else i for i in seg['ids']], -1.0)
  assert 'outside the vocabulary' in no_flag['error']                 # without the argument a `*` stays the error it is
  words = text.lower().split()[2:]
  for e in (r, seg):
    assert e['error'] is None and e['text'] == star_text.lower() and e['ids'][0] == alignment.WILDCARD
    assert e['ids'].count(alignment.WILDCARD) == 1 and len(e['gaps']) == 1 and len(e['fit']) == len(e['ids'])
    timed = alignment.timed_words(e['ids'], e['spans'], e['sample_rate'], e['seconds'], concat=alignment.concat_of(e), fit=e['fit'])
    assert [w['word'] for w in timed] == words and len(e['word_fit']) == len(words)
    g = e['gaps'][0]
    assert 0.0 <= g['start'] <= g['end'] <= timed[0]['start']
    prev = g['end']
    for w in timed:
      assert prev <= w['start'] <= w['end'] <= e['seconds'] and w['fit'] <= 0.0
      prev = w['end']
    a, b = e['spans'][0]
    assert e['fit'][0] == -1.0 * (b - a) and all(f <= 0.0 for f in e['fit'])
    line = alignment.result_json(e)
    assert line['gaps'] == e['gaps'] and line['words'] == timed and 'fit' in line['words'][0]
  assert (again['spans'] == r['spans']).all() and again['score'] == r['score'] and again['fit'] == r['fit']
  assert ends['error'] is None and ends['ids'][0] == ends['ids'][-1] == alignment.WILDCARD and len(ends['gaps']) == 2
  assert 'fit' not in ends and ends['gaps'][0]['end'] <= ends['gaps'][1]['start']
  assert res[2] == 0 and (host[0] == seg['spans']).all() and host[1] == seg['score'] and host[3].tolist() == seg['fit']
  # the CLI: the same words, gaps and fits, and no directory
  cwd = tmp_path / 'cwd'
  cwd.mkdir()
  out = tmp_path / 'wild.jsonl'
  base = ['--train-dir', str(train), '--run-name', 'run', '--device', dev]
  run = lambda args: subprocess.run([sys.executable, os.path.join(ROOT, 'speecht-cli'), 'align'] + base + args, capture_output=True,
                                    text=True, timeout=600, cwd=str(cwd))
  c = run([str(audio), '--segment', '--mask-padding', '--fit', '--output', str(out), '--wildcard'])
  assert c.returncode == 0, c.stderr
  rec, = [json.loads(l) for l in out.read_text().splitlines()]
  assert rec['words'] == alignment.result_json(seg)['words'] and rec['gaps'] == seg['gaps'] and rec['score'] == seg['score']
  rows = [l.split('\t') for l in c.stdout.splitlines()]
  assert [row[3] for row in rows] == ['*'] + words and rows[0][4] == '-'
  assert [float(row[4]) for row in rows[1:]] == [float('{:.4f}'.format(w['fit'])) for w in rec['words']]
  assert sorted(os.listdir(str(cwd))) == []
