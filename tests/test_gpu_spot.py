"""Keyword spotting on the GPU: st_ctc_spot_f32 against its host form (st_ctc_spot_host -- the two share their arithmetic,
csrc/ctc_spot_core.h) BIT FOR BIT on score, span, status and both traces, through every states-per-lane dispatch, the frame
counts at the edges of the 64-frame chunks and the class counts 2, 29 and 32; `engine.spot`, `inference.spot`, `spot_files` and
the command line on top of it.

The host form equals the float64 specification (tests/spot_oracle.py) exactly: tests/test_spot_cpu.py."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import align_oracle as AO
from tests import spot_oracle as SO
from tests import workloads as WL
from tests.test_spot_cpu import DISPATCH_LENGTHS, all_jobs, assert_same_bits, csr, dispatch_case, edge_batch, host_spot

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_FLAC = os.path.join(ROOT, 'tests', 'golden', '1089-134686-0037.flac')
C_PITCH = 32


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def device_spot(dev, logits, seq_lens, keywords, jobs, max_keyword_len=None, trace=True, halo=0, slack=0, poison=False):
  """st_ctc_spot_f32 on a dense [B, T, C] batch laid out as padded NWC (c_pitch 32, the pitch columns 1e30; ``halo`` rows before
  and ``halo + slack`` rows behind each utterance's frames) -> (score, span, status, trace_score, trace_start) as `host_spot`.
  ``poison``: NaN in the halo and slack rows and in every row past its utterance's seq_len -- none of them may be read into a result."""
  from speecht_amd import _lib
  from speecht_amd._lib import Tensor3
  lib = _lib.load()
  B, T, C = logits.shape
  t_pitch = T + 2 * halo + slack
  ids, offs = csr(keywords)
  n = len(jobs)
  table = np.array([j for job in jobs for j in job] + [0, 0], dtype=np.int32)
  max_len = max([len(k) for k in keywords] + [1]) if max_keyword_len is None else max_keyword_len
  x = torch.full((B, t_pitch, C_PITCH), 1e30, dtype=torch.float32, device=dev)         # the pitch columns must never be read
  x[:, halo:halo + T, :C] = torch.as_tensor(np.ascontiguousarray(logits, dtype=np.float32))
  if poison:
    x[:, :halo] = float('nan')
    x[:, halo + T:] = float('nan')
    for b, n_b in enumerate(seq_lens):
      x[b, halo + min(max(int(n_b), 0), T):] = float('nan')
  to = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
  d_ids, d_offs, d_lens, d_jobs = to(ids), to(offs), to(np.asarray(seq_lens, dtype=np.int32)), to(table)
  # a sentinel row behind every output
  score = torch.full((n + 1,), 7.0, dtype=torch.float64, device=dev)
  span = torch.full((n + 1, 2), -7, dtype=torch.int32, device=dev)
  status = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
  trace_score = torch.full((n + 1, T), 7.0, dtype=torch.float64, device=dev)
  trace_start = torch.full((n + 1, T), -7, dtype=torch.int32, device=dev)
  need = lib.st_ctc_spot_ws(B, T, max_len, n)
  assert need == (B * T * 256 + 512 if 1 <= max_len <= 511 else 0)           # (0: arguments the entry point refuses)
  ws = torch.empty(need // 4 + 4, dtype=torch.int32, device=dev)
  P = lambda t: ctypes.c_void_p(t.data_ptr())
  desc = Tensor3(x.data_ptr(), B, T, C, halo, t_pitch, C_PITCH)
  _lib.call('st_ctc_spot_f32', ctypes.byref(desc), P(d_lens), P(d_ids), P(d_offs), len(keywords), max_len, P(d_jobs), n, P(score), P(span),
            P(trace_score) if trace else None, P(trace_start) if trace else None, P(status), P(ws), need,
            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
  torch.cuda.synchronize()
  score, span, status = score.cpu().numpy(), span.cpu().numpy(), status.cpu().numpy()
  trace_score, trace_start = trace_score.cpu().numpy(), trace_start.cpu().numpy()
  assert score[-1] == 7.0 and (span[-1] == -7).all() and status[-1] == -7             # nothing written past the outputs
  assert (trace_score[-1] == 7.0).all() and (trace_start[-1] == -7).all()
  if not trace:
    assert (trace_score == 7.0).all() and (trace_start == -7).all()
    return score[:n], span[:n], status[:n], None, None
  return score[:n], span[:n], status[:n], trace_score[:n], trace_start[:n]


@pytest.mark.parametrize('L', DISPATCH_LENGTHS)
def test_kernel_equals_host_form_at_every_dispatch(dev, L):
  logits, lens, keywords, jobs, planted = dispatch_case(L, 29)
  want = host_spot(logits, lens, keywords, jobs)
  got = device_spot(dev, logits, lens, keywords, jobs)
  assert_same_bits(got, want)
  assert got[0][6] == 0.0 and tuple(got[1][6]) == planted and got[0][8] == -np.inf
  # without the trace, and in a padded layout whose halo rows and rows past each seq_len are poisoned: the same bits
  assert_same_bits(device_spot(dev, logits, lens, keywords, jobs, trace=False), want[:3] + (None, None))
  assert_same_bits(device_spot(dev, logits, lens, keywords, jobs, halo=3, slack=5, poison=True), want)


def chunk_edge_case(T, C):
  """Four utterances of T frames' room -- full, one frame short, half, empty -- and keywords of 1 .. 6 ids, one with equal
  neighbours, one planted in the first utterance."""
  rng = np.random.default_rng(100 * T + C)
  planted = AO.random_labels(rng, min(3, T), C, repeat_prob=0.0)
  keywords = [planted, [0], [0, 0], AO.random_labels(rng, 6, C, 0.3), AO.random_labels(rng, 4, C, 0.0)]
  lens = np.array([T, T - 1, T // 2, 0], dtype=np.int32)
  xs = [AO.planted_logits(rng, planted, T, C)[0] if T >= AO.min_frames(planted) else AO.random_logits(rng, T, C, 1.0)]
  xs += [AO.random_logits(rng, int(n), C, scale) for n, scale in zip(lens[1:], (0.05, 4.0, 1.0))]
  return AO.pad_batch(xs, T)[0], lens, keywords, all_jobs(4, len(keywords))


@pytest.mark.parametrize('C', [2, 29, 32])
@pytest.mark.parametrize('T', [1, 2, 63, 64, 65, 128, 129])
def test_chunk_edges_and_class_counts(dev, T, C):
  logits, lens, keywords, jobs = chunk_edge_case(T, C)
  want = host_spot(logits, lens, keywords, jobs)
  assert_same_bits(want, SO.spot_batch(logits, lens, keywords, jobs))
  assert_same_bits(device_spot(dev, logits, lens, keywords, jobs), want)
  assert_same_bits(device_spot(dev, logits, lens, keywords, jobs, trace=False), want[:3] + (None, None))
  assert_same_bits(device_spot(dev, logits, lens, keywords, jobs, halo=3, slack=2, poison=True), want)
  assert (want[2] == 0).all() and np.isfinite(want[0][1])


def test_edge_cases_job_tables_and_refusals(dev):
  from speecht_amd import _lib
  # equal neighbours, all-equal logits, single -inf classes, a keyword that does not fit, seq_len 0
  x, lens, keywords, jobs = edge_batch()
  want = host_spot(x, lens, keywords, jobs)
  assert_same_bits(device_spot(dev, x, lens, keywords, jobs), want)
  # the same pair twice, pairs out of order, pairs outside the tables: each job is its own, in table order
  rng = np.random.default_rng(13)
  table = [jobs[i] for i in rng.permutation(len(jobs))[:20]] + [jobs[3], jobs[3], (7, 0), (-1, 0), (0, 5), (0, -1), jobs[0]]
  got = device_spot(dev, x, lens, keywords, table)
  assert_same_bits(got, host_spot(x, lens, keywords, table))
  index = {job: i for i, job in enumerate(jobs)}
  for i, job in enumerate(table):
    if job in index:
      assert_same_bits(tuple(a[i:i + 1] for a in got), tuple(a[index[job]:index[job] + 1] for a in want))
    else:
      assert got[2][i] == 1 and got[0][i] == -np.inf and (got[1][i] == -1).all()
      assert (got[3][i] == -np.inf).all() and (got[4][i] == -1).all()
  # lengths outside 0 .. frames and a keyword beyond the dispatch are refused per job
  bad = lens.copy()
  bad[0], bad[2] = x.shape[1] + 1, -3
  got = device_spot(dev, x, bad, keywords, jobs, max_keyword_len=31)
  assert_same_bits(got, host_spot(x, bad, keywords, jobs, max_keyword_len=31))
  assert [int(s) for s in got[2]] == [int(b in (0, 2) or k == 4) for b, k in jobs]
  # no jobs: valid, nothing is written; bad arguments are errors
  assert len(device_spot(dev, x, lens, keywords, [])[0]) == 0
  with pytest.raises(_lib.SpeechtHipError):
    device_spot(dev, x, lens, keywords, jobs, max_keyword_len=512)
  with pytest.raises(_lib.SpeechtHipError):
    device_spot(dev, x, lens, keywords, jobs, max_keyword_len=0)


@pytest.fixture(scope='module')
def engine_case(dev):
  """A small network whose random weights decode 3 to 9 characters per utterance (as tests/test_gpu_align.py), four utterances."""
  from speecht_amd.engine import Wav2LetterEngine
  layers = WL.w2l_layers(16, width=40, fc=72)
  params = WL.xavier_params(layers, seed=21, bias_range=0.3)
  params[-1] = (params[-1][0] * 100.0, params[-1][1] * 0.0)
  lengths = [260, 201, 124, 77]
  feats = [WL.synthetic_features(300 + i, t, 16).astype(np.float32) for i, t in enumerate(lengths)]
  eng = Wav2LetterEngine(layers, device=dev)
  eng.set_weights(params)
  return eng, feats, lengths


def _load(eng, feats, lengths):
  x = np.zeros((len(feats), max(lengths), 16), dtype=np.float32)
  for b, f in enumerate(feats):
    x[b, :f.shape[0]] = f
  eng.load_batch(x, lengths)
  eng.forward()
  return eng.logits_time_major().cpu().numpy().transpose(1, 0, 2)


def test_engine_spot_equals_the_oracle_and_align(engine_case):
  eng, feats, lengths = engine_case
  logits = _load(eng, feats, lengths)
  ids, _ = eng.greedy_decode()
  assert all(len(s) >= 2 for s in ids)
  lens = [n // 2 for n in lengths]
  # the decoded ids of every utterance, one long phrase (another dispatch group) and short ones
  rng = np.random.default_rng(14)
  keywords = [list(s) for s in ids] + [AO.random_labels(rng, 40, 29, 0.1), [int(ids[0][0])], list(ids[1][:2])]
  score, spans, status, tr_score, tr_start = eng.spot(keywords, trace=True)
  jobs = all_jobs(len(ids), len(keywords))
  want = SO.spot_batch(logits, lens, keywords, jobs)
  assert_same_bits((score, spans, status, tr_score, tr_start), want)
  plain = eng.spot(keywords)
  assert len(plain) == 3
  assert_same_bits(plain + (None, None), want[:3] + (None, None))
  # a job table of its own, out of order and with a repeat, through the same grouping
  table = [(3, 4), (0, 0), (2, 6), (0, 0), (1, 4), (9, 0), (0, 99)]
  assert_same_bits(eng.spot(keywords, jobs=table, trace=True), SO.spot_batch(logits, lens, keywords, table))
  # the whole label as the keyword: score 0, and the span of `align` from its first label's first frame to its last label's end
  al_spans, _, al_status = eng.align(ids)
  K = len(keywords)
  for b, lab in enumerate(ids):
    assert al_status[b] == 0 and score[b * K + b] == 0.0
    assert tuple(spans[b * K + b]) == (al_spans[b][0, 0], al_spans[b][-1, 1])
  # a trace call split over jobs gives the same arrays
  from speecht_amd import engine_decode
  old = engine_decode.SPOT_TRACE_BYTES
  engine_decode.SPOT_TRACE_BYTES = 12 * logits.shape[1] * 5
  try:
    assert_same_bits(eng.spot(keywords, trace=True), want)
  finally:
    engine_decode.SPOT_TRACE_BYTES = old
  # refused on the host: empty, too long, ids outside the classes
  for bad in ([[]], [[1] * 512], [[28]], [[-1]]):
    with pytest.raises(ValueError):
      eng.spot(bad)
  assert len(eng.spot([])[0]) == 0 and len(eng.spot(keywords, jobs=[])[0]) == 0


def test_inference_spot_alone_and_in_masked_batches(engine_case):
  from speecht_amd import inference, spotting
  eng, feats, lengths = engine_case
  solo_ids = inference.transcribe(eng, feats, batch_size=1)[0]
  assert all(len(s) >= 2 for s in solo_ids)
  keywords = [list(s) for s in solo_ids] + [list(solo_ids[0][:2]), [27], [0, 1]]
  one = inference.spot(eng, feats, keywords, batch_size=1, trace=True)
  four = inference.spot(eng, feats, keywords, batch_size=4, mask_padding=True, trace=True)
  assert one[0].shape == (4, len(keywords)) and one[1].shape == (4, len(keywords), 2) and (one[2] == 0).all() and (four[2] == 0).all()
  # alone: bit for bit the oracle on the logits the utterance gets alone
  for i, f in enumerate(feats):
    logits = _load(eng, [f], [lengths[i]])
    want = SO.spot_batch(logits, [lengths[i] // 2], keywords, all_jobs(1, len(keywords)))
    want = want[:3] + (want[3][:, :lengths[i] // 2], want[4][:, :lengths[i] // 2])          # the utterance's own output frames
    assert_same_bits((one[0][i], one[1][i], one[2][i], one[3][i], one[4][i]), want)
    assert one[0][i, i] == 0.0                                             # its own transcript is spelled by the greedy classes
  # in a masked batch: the same hits (the logits agree to the rounding of two summation orders)
  assert np.array_equal(one[1], four[1])
  finite = np.isfinite(one[0])
  assert np.array_equal(finite, np.isfinite(four[0])) and np.allclose(one[0][finite], four[0][finite], rtol=1e-5, atol=1e-5)
  for i in range(len(feats)):
    for k in range(len(keywords)):
      a, b = (spotting.pick_hits(r[3][i][k], r[4][i][k], -0.69) for r in (one, four))
      assert [h[:2] for h in a] == [h[:2] for h in b]
      assert np.allclose([h[2] for h in a], [h[2] for h in b], rtol=1e-5, atol=1e-5)
  assert inference.spot(eng, [], keywords)[0].shape == (0, len(keywords)) and inference.spot(eng, feats, [])[0].shape == (4, 0)


def _oracle_traces(model, path, keywords):
  """The oracle's result for every keyword on the logits the engine computes for one file, and the file's duration."""
  from speecht_amd import spotting, transcription
  samples, rate = transcription.load_native(path)
  feats = transcription.device_features([samples], [rate], 'power', 22050, model.engine.device)
  model.engine.load_batch(feats[0][None], [feats[0].shape[0]])
  model.engine.forward()
  logits = model.engine.logits_time_major().cpu().numpy()[:feats[0].shape[0] // 2, 0]
  return [SO.spot64(logits, spotting.keyword_ids(k)) for k in keywords], len(samples) / float(rate)


def _expected_hits(traces, keywords, seconds, threshold, all_hits):
  """What `spot_files` must report for one file."""
  from speecht_amd.alignment import frames_to_seconds
  sec = lambda f: round(frames_to_seconds(f, 22050, 160, seconds), 4)
  hits = []
  for n, (k, r) in enumerate(zip(keywords, traces)):
    found = SO.pick_hits(r['trace_score'], r['trace_start'], threshold) if all_hits else \
        [h for h in [(r['span'][0], r['span'][1], r['score'])] if np.isfinite(h[2]) and h[2] / (h[1] - h[0]) >= threshold]
    hits += [(sec(a), sec(e), n, dict(keyword=k, start=sec(a), end=sec(e), score=s, score_per_frame=s / (e - a))) for a, e, s in found]
  return [h[3] for h in sorted(hits, key=lambda h: h[:3])]


def _fresh_model(tmp_path):
  from speecht_amd.speech_input import SingleInputLoader
  from speecht_amd.speech_model import Wav2LetterModel
  model = Wav2LetterModel(SingleInputLoader(128), 128, 29)
  model.add_training_ops()
  model.add_decoding_ops()
  model.finalize(str(tmp_path / 'log'), 'r', 'record')
  model.init_seed = 1234
  return model


KEYWORDS = ['the', ' a ', 'new york', "don't"]


def test_spot_files_and_cli_on_the_golden_flac(dev, tmp_path):
  from speecht_amd import segmentation, spotting
  from speecht_amd.speech_model import Session
  model = _fresh_model(tmp_path)
  train = tmp_path / 'train'
  (train / 'run').mkdir(parents=True)
  missing = str(tmp_path / 'nothing.flac')
  with Session(dev) as sess:
    model.init_session(sess)
    model.saver.save(sess, str(train / 'run' / 'speechT'), global_step=model.global_step)
    traces, seconds = _oracle_traces(model, GOLDEN_FLAC, KEYWORDS)
    # the best hits whatever they score; every hit above the median score per frame of all the oracle's hits
    lowest = -1e9
    per_frame = [h['score_per_frame'] for h in _expected_hits(traces, KEYWORDS, seconds, -np.inf, True)]
    threshold = round(float(np.median(per_frame)), 4)
    best = _expected_hits(traces, KEYWORDS, seconds, lowest, False)
    every = _expected_hits(traces, KEYWORDS, seconds, threshold, True)
    res = spotting.spot_files(model.engine, [GOLDEN_FLAC, missing], KEYWORDS, threshold=lowest)
    res_all = spotting.spot_files(model.engine, [GOLDEN_FLAC], KEYWORDS, threshold=threshold, all_hits=True)
    seg = spotting.spot_files(model.engine, [GOLDEN_FLAC], KEYWORDS, threshold=threshold, all_hits=True, batch_size=4, mask_padding=True,
                              segment=segmentation.SegmentOptions(min_silence=0.1, max_segment=2.0))
  assert [r['path'] for r in res] == [GOLDEN_FLAC, missing] and 'no such file' in res[1]['error'] and res[1]['hits'] is None
  assert res[0]['error'] is None and res[0]['seconds'] == seconds
  assert res[0]['hits'] == best and res_all[0]['hits'] == every
  assert len(best) == len(KEYWORDS) and 1 < len(every) < len(per_frame)
  for hits in (every, seg[0]['hits']):
    for k in KEYWORDS:                                                    # the hits of a keyword do not overlap, and lie inside the file
      mine = [h for h in hits if h['keyword'] == k]
      assert all(0.0 <= h['start'] <= h['end'] <= seconds and h['score'] <= 0.0 and h['score_per_frame'] >= threshold for h in mine)
      assert all(mine[i]['end'] <= mine[i + 1]['start'] for i in range(len(mine) - 1))
    assert [(h['start'], h['end']) for h in hits] == sorted((h['start'], h['end']) for h in hits)
  assert len(seg[0]['hits']) >= 1
  # the command line: the same lines, the JSON lines, the unreadable file on stderr and in the exit status
  kw_file = tmp_path / 'kw.txt'
  kw_file.write_text('# keywords\n' + '\n'.join(KEYWORDS) + '\nTHE\n')
  cwd = tmp_path / 'cwd'
  cwd.mkdir()
  out = tmp_path / 'spot.jsonl'
  base = ['--train-dir', str(train), '--run-name', 'run', '--device', dev]
  run = lambda args: subprocess.run([sys.executable, os.path.join(ROOT, 'speecht-cli'), 'spot'] + base + args, capture_output=True,
                                    text=True, timeout=600, cwd=str(cwd))
  r = run(['--threshold', str(lowest), '--keywords', str(kw_file), '--output', str(out), GOLDEN_FLAC, missing])
  assert r.returncode == 1 and 'nothing.flac: no such file' in r.stderr, r.stderr
  line = lambda h: '{}\t{:.3f}\t{:.3f}\t{}\t{:.4f}\t{:.4f}'.format(GOLDEN_FLAC, h['start'], h['end'], h['keyword'], h['score'], h['score_per_frame'])
  assert r.stdout.splitlines() == [line(h) for h in best]
  rec, = [json.loads(l) for l in out.read_text().splitlines()]
  assert rec == dict(path=GOLDEN_FLAC, seconds=seconds, hits=best)
  assert sorted(os.listdir(str(cwd))) == []
  r2 = run(['--all', '--threshold', str(threshold)] + [a for k in KEYWORDS for a in ('--keyword', k)] + [GOLDEN_FLAC])
  assert r2.returncode == 0 and r2.stdout.splitlines() == [line(h) for h in every], r2.stderr
