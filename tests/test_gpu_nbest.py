"""N-best lists of both CTC beam searches on the GPU (st_ctc_beam_search_decode_nbest / _lm_nbest: the NBEST tail of
ctc_beam_kernel) against the float64 specification of tests/nbest_oracle.py, the sentence-score kernel (st_lm_score_prefixes_f64)
bit for bit against its host form, second-pass rescoring against the oracle's, and the layers above -- transcribe, the CLI.

The comparison with the oracle (nbest_oracle.check_list): the number of hypotheses exact; every returned prefix in the oracle's
final set with its score within rtol = atol = 1e-4 (what test_gpu_lm_beam.py holds the top path to); order and membership exact
except among oracle scores within 1e-4 of each other.  tests/test_nbest_cpu.py shows on the oracle alone that such near ties are
rare in these cases and that the sets do not change when the oracle runs in float32."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lm_oracle as L
from tests import nbest_oracle as N
from tests import test_nbest_cpu as C
from tests import workloads as WL
from tests.test_lm_oracle_cpu import word_logits

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = C.TINY
GOLDEN_FLAC = os.path.join(ROOT, 'tests', 'golden', '1089-134686-0037.flac')


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def _engine(dev, logits, lens):
  from speecht_amd.engine import Wav2LetterEngine
  T, B, Cn = logits.shape
  eng = Wav2LetterEngine([(1, 1, 16, Cn, False)], device=dev)
  eng.load_batch(np.zeros((B, T, 16)), [T] * B)
  eng.X[-1].interior().copy_(torch.as_tensor(np.transpose(logits, (1, 0, 2)).astype(np.float32)))
  eng.ctc_lens = torch.as_tensor(np.asarray(lens).astype(np.int32)).to(dev)
  return eng


def _check(lists, sets, n):
  assert len(lists) == len(sets)
  for b, (got, entries) in enumerate(zip(lists, sets)):
    try:
      N.check_list(got, entries, n)
    except AssertionError as e:
      raise AssertionError('utterance {}: {}'.format(b, e)) from e


@pytest.mark.parametrize('case,n', [(c, n) for c in C.FREE_CASES for n in C.n_bests(c[0])])
def test_lm_free_lists_match_the_oracle(dev, case, n):
  from speecht_amd._lib import launch_trace
  beam, classes, transform = case
  logits, lens = C.gpu_case(C.case_seed(case, 'free'), classes)
  eng = _engine(dev, logits, lens)
  with launch_trace() as tr:
    lists = eng.beam_search_decode_nbest(n, beam, transform)
  assert any(l.startswith('ctc_beam<{}>'.format('wide' if beam > 64 else 'wave')) and l.endswith('nbest={}'.format(n)) for l in tr.lines), tr.lines
  sets = C.oracle_sets('free', case)
  assert [len(l) for l in lists] == [min(n, len(e)) for e in sets]                 # (a), the rows of length 0 and 1 included
  assert len(lists[3]) == 1 and lists[3][0] == ([], 0.0) and len(lists[4]) == min(n, beam, classes)
  _check(lists, sets, n)


@pytest.mark.parametrize('case,n', [(c, n) for c in C.LM_CASES for n in C.n_bests(c[0])])
def test_lm_lists_match_the_oracle(dev, tmp_path_factory, case, n):
  from speecht_amd._lib import launch_trace
  beam, order, transform = case
  lm = C.library_model(tmp_path_factory, order)
  logits, lens = C.gpu_case(C.case_seed(case, 'lm'))
  eng = _engine(dev, logits, lens)
  with launch_trace() as tr:
    lists = eng.lm_beam_search_decode_nbest(lm, n, beam, transform)
  assert any(l.startswith('ctc_beam_lm<') and 'order={}'.format(order) in l and l.endswith('nbest={}'.format(n)) for l in tr.lines), tr.lines
  sets = C.oracle_sets('lm', case)
  assert [len(l) for l in lists] == [min(n, len(e)) for e in sets]
  assert len(lists[3]) == 1 and lists[3][0][0] == [] and len(lists[4]) == min(n, beam, 29)
  _check(lists, sets, n)


@pytest.mark.parametrize('beam', [1, 16, 100])
def test_one_best_is_the_top_path_bit_for_bit(dev, beam):
  from speecht_amd.language_model import LanguageModel
  logits, lens = C.gpu_case(beam)
  eng = _engine(dev, logits, lens)
  lm = LanguageModel.load(TINY)
  for transform in (None, 'log10_softmax'):
    ids, logp = eng.beam_search_decode(beam, transform)
    lists = eng.beam_search_decode_nbest(1, beam, transform)
    assert [len(l) for l in lists] == [1] * 5
    assert [l[0][0] for l in lists] == ids
    assert np.array_equal(np.array([l[0][1] for l in lists], dtype=np.float32), logp[:, 0])
    ids, logp = eng.lm_beam_search_decode(lm, beam, transform)
    lists = eng.lm_beam_search_decode_nbest(lm, 1, beam, transform)
    assert [l[0][0] for l in lists] == ids
    assert np.array_equal(np.array([l[0][1] for l in lists], dtype=np.float32), logp[:, 0])


def _raw_nbest(eng, dev, beam, n, max_out, lm=None):
  """The entry points themselves with a `max_out` of the caller's: (ids [B, n, max_out], lens [B, n], log_prob [B, n], n_hyps [B])
  over buffers filled with a pattern, so that what the kernel leaves alone shows."""
  from speecht_amd import _lib
  lib = _lib.load()
  B = eng.dec_lens.numel()
  ws = torch.empty(lib.st_ctc_beam_ws(B, eng.t_out, beam) // 4 + 16, dtype=torch.int32, device=dev)
  ids = torch.full((B, n, max_out), -7, dtype=torch.int32, device=dev)
  lens = torch.full((B, n), -7, dtype=torch.int32, device=dev)
  logp = torch.full((B, n), 7.0, dtype=torch.float32, device=dev)
  count = torch.full((B,), -7, dtype=torch.int32, device=dev)
  eng._wait_uploads()
  torch.cuda.synchronize()
  tail = (eng._ptr(ids), max_out, eng._ptr(lens), eng._ptr(logp), eng._ptr(count), eng._ptr(ws), ws.numel() * 4, eng.stream_ptr)
  if lm is None:
    _lib.call('st_ctc_beam_search_decode_nbest', eng.X[-1].ref, eng._ptr(eng.ctc_lens), beam, 0, n, *tail)
  else:
    _lib.call('st_ctc_beam_search_decode_lm_nbest', eng.X[-1].ref, eng._ptr(eng.ctc_lens), beam, 1, lm.device_handle(dev),
              ctypes.c_float(0.8), ctypes.c_float(0.0), ctypes.c_float(2.3), ctypes.c_float(-1000.0), n, *tail)
  torch.cuda.synchronize()
  return ids.cpu().numpy(), lens.cpu().numpy(), logp.cpu().numpy(), count.cpu().numpy()


@pytest.mark.parametrize('with_lm', [False, True])
def test_truncated_labels_and_unused_slots(dev, with_lm):
  from speecht_amd import _lib
  from speecht_amd.language_model import LanguageModel
  lm = LanguageModel.load(TINY) if with_lm else None
  logits, lens = C.gpu_case(77)
  eng = _engine(dev, logits, lens)
  beam, n = 100, 70                                          # two rounds of chain walks
  full = _raw_nbest(eng, dev, beam, n, eng.t_out, lm)
  cut = _raw_nbest(eng, dev, beam, n, 3, lm)
  assert np.array_equal(full[1], cut[1]) and np.array_equal(full[2], cut[2]) and np.array_equal(full[3], cut[3])
  assert full[3].tolist() == [70, 70, 70, 1, 29] and full[1].max() > 3              # out_lens reports the true length
  for b in range(5):
    for h in range(n):
      if h < full[3][b]:
        k = min(int(full[1][b, h]), 3)
        assert np.array_equal(cut[0][b, h, :k], full[0][b, h, :k]) and (cut[0][b, h, k:] == -7).all()
        assert (full[0][b, h, full[1][b, h]:] == -7).all() and np.isfinite(full[2][b, h])
      else:                                                  # unused slots: length 0, -inf, no label written
        assert full[1][b, h] == 0 and full[2][b, h] == -np.inf and (full[0][b, h] == -7).all()
  # n_best outside 1..beam is refused
  for bad in (0, beam + 1):
    with pytest.raises(_lib.SpeechtHipError, match='n_best'):
      _raw_nbest(eng, dev, beam, bad, 3, lm)
  with pytest.raises(ValueError, match='n_best'):
    eng.beam_search_decode_nbest(17, 16)


@pytest.mark.parametrize('order,seed', [(3, None), (5, 905)])
def test_device_sentence_scores_are_the_host_form_bit_for_bit(dev, tmp_path_factory, order, seed):
  lm = C.library_model(tmp_path_factory, order, seed)
  logits, lens = C.gpu_case(31)
  eng = _engine(dev, logits, lens)
  prefixes = C.hand_made_prefixes(np.random.default_rng(5))
  prefixes += [ids for l in eng.beam_search_decode_nbest(100, 100) for ids, _ in l]
  prefixes += [ids for l in eng.lm_beam_search_decode_nbest(lm, 64, 64) for ids, _ in l]
  assert len(prefixes) > 300
  g, nw, nv = eng.lm_score_prefixes(lm, prefixes)
  hg, hw, hv = C.score_host(lm, prefixes)
  assert np.array_equal(g.view(np.int64), hg.view(np.int64)) and np.array_equal(nw, hw) and np.array_equal(nv, hv)
  ref = C.oracle_model(order, seed)
  for i in (0, 1, 4, 12, len(prefixes) - 1):
    rg, rw, rv = N.sentence_score(ref, prefixes[i])
    assert g[i] == pytest.approx(rg, rel=1e-12) and (nw[i], nv[i]) == (rw, rv)
  empty = eng.lm_score_prefixes(lm, [])
  assert len(empty[0]) == 0
  with pytest.raises(ValueError, match='0..27'):
    eng.lm_score_prefixes(lm, [[1, 28]])


def test_rescoring_equals_the_oracle(dev, tmp_path_factory):
  from speecht_amd import nbest
  case = (16, 3, 'log10_softmax')
  assert case in C.LM_CASES
  beam, order, transform = case
  first = (0.8, 0.0, 2.3)
  lm, ref = C.library_model(tmp_path_factory, 3), C.oracle_model(3)
  lm2, ref2 = C.library_model(tmp_path_factory, 4), C.oracle_model(4)             # a random order-4 model holding the sentence words
  logits, lens = C.gpu_case(C.case_seed(case, 'lm'))
  eng = _engine(dev, logits, lens)
  lists = nbest.components(eng, lm, eng.lm_beam_search_decode_nbest(lm, beam, beam, transform), first)
  sets = C.oracle_sets('lm', case)
  # the first pass's own model and weights: its own scores and order (a pair may swap only on equal float32 scores)
  order_same, scores_same = nbest.rescore(lists, eng, lm, *first)
  for hyps, order_b, scores_b in zip(lists, order_same, scores_same):
    lp = np.array([h['log_prob'] for h in hyps])
    np.testing.assert_allclose(scores_b, lp[order_b], rtol=0, atol=1e-9)
    assert all(i < j or lp[i] == lp[j] for i, j in zip(order_b, order_b[1:]))
    assert sorted(order_b) == list(range(len(hyps)))
  for model, oracle, weights in ((lm, ref, (1.7, -0.4, 0.6)), (lm2, ref2, (0.8, 0.0, 2.3)), (lm2, ref2, (2.5, 0.3, -0.5))):
    orders, scores = nbest.rescore(lists, eng, model, *weights)
    for hyps, entries, order_b, scores_b in zip(lists, sets, orders, scores):
      want_order, want_scores = N.rescore(N.split(ref, [(list(pre), total) for pre, total, _ in entries], *first), oracle, *weights)
      want = [(entries[i][0], s, None) for i, s in zip(want_order, want_scores)]
      N.check_list([(hyps[i]['ids'], s) for i, s in zip(order_b, scores_b)], want, len(want))


def test_a_second_model_changes_the_winner(dev):
  """The acoustics favour 'the kat'; an LM-free first pass returns it first, with 'the cat' further down its list, and the second
  pass under the tiny model puts 'the cat' first -- as the oracle's rescoring of the oracle's list does."""
  from speecht_amd import nbest
  from speecht_amd.language_model import LanguageModel
  rng = np.random.default_rng(7)
  x = word_logits('the kat', rng, noise=0.3)
  k, c = L.LETTERS.index('k'), L.LETTERS.index('c')
  for t in range(len(x)):
    if x[t].argmax() == k:
      x[t, c] = x[t, k] - 0.5
  eng = _engine(dev, x[:, None, :].astype(np.float32), [len(x)])
  lm = LanguageModel.load(TINY)
  lists = nbest.components(eng, None, eng.beam_search_decode_nbest(16, 16))
  assert L.ids_to_text(lists[0][0]['ids']) == 'the kat' and lists[0][0]['acoustic'] == lists[0][0]['log_prob']
  again = nbest.rescored(lists, eng, lm, 0.8, 0.0, 2.3)
  assert L.ids_to_text(again[0][0]['ids']) == 'the cat' and again[0][0]['first_pass_rank'] > 0
  assert again[0][0]['words'] == 2 and again[0][0]['valid_words'] == 2
  entries = N.final_sets(x[:, None, :], [len(x)], 16)[0]
  want_order, want_scores = N.rescore([(list(pre), total) for pre, total, _ in entries], L.ArpaModel.load(TINY), 0.8, 0.0, 2.3)
  assert L.ids_to_text(entries[want_order[0]][0]) == 'the cat'
  N.check_list([(h['ids'], h['log_prob']) for h in again[0]], [(entries[i][0], s, None) for i, s in zip(want_order, want_scores)], 16)


def test_transcribe_with_lists_returns_the_same_best_ids(dev):
  from speecht_amd.engine import Wav2LetterEngine
  from speecht_amd.inference import transcribe
  layers = WL.w2l_layers(16, width=40, fc=72)
  params = WL.xavier_params(layers, seed=21, bias_range=0.3)
  params[-1] = (params[-1][0] * 12.0, params[-1][1] * 4.0)
  rng = np.random.default_rng(8)
  lengths = rng.integers(60, 260, 6).tolist()
  feats = [WL.synthetic_features(300 + i, t, 16).astype(np.float32) for i, t in enumerate(lengths)]
  eng = Wav2LetterEngine(layers, device=dev)
  eng.set_weights(params)
  opts = dict(lm_weight=2.0, valid_word_count_weight=1.0)
  for decode in (dict(beam_width=32), dict(beam_width=32, language_model=TINY, lm_options=opts)):
    plain = transcribe(eng, feats, batch_size=4, pipeline=False, **decode)
    ids, texts, lists = transcribe(eng, feats, batch_size=4, nbest=4, **decode)
    assert ids == plain[0] and texts == plain[1] and any(len(s) > 0 for s in ids)
    for i, hyps in enumerate(lists):
      assert 1 <= len(hyps) <= 4 and hyps[0]['ids'] == ids[i] and hyps[0]['text'] == texts[i]
      assert all(('lm_log10' in h) == ('language_model' in decode) and 'acoustic' in h for h in hyps)
      assert all(a['log_prob'] >= b['log_prob'] for a, b in zip(hyps, hyps[1:]))
  # with a second pass the best hypothesis is the rescored winner, and spans / confidences belong to it
  res = transcribe(eng, feats, batch_size=4, beam_width=32, nbest=4, rescore=dict(language_model=TINY, lm_weight=3.0),
                   timestamps=True, confidence=True)
  assert len(res) == 5
  for i, hyps in enumerate(res[4]):
    assert hyps[0]['ids'] == res[0][i] and sorted(h['first_pass_rank'] for h in hyps) == list(range(len(hyps)))
    assert res[2][i] is None or len(res[2][i]) == len(res[0][i])
  assert transcribe(eng, [], beam_width=4, nbest=2) == ([], [], [])


def test_command_line_prints_the_lists(dev, tmp_path):
  from speecht_amd.speech_model import Session
  from tests.test_gpu_confidence import _golden_model
  model = _golden_model(tmp_path)
  train = tmp_path / 'train'
  (train / 'run').mkdir(parents=True)
  with Session(dev) as sess:
    model.init_session(sess)
    model.saver.save(sess, str(train / 'run' / 'speechT'), global_step=model.global_step)
  base = ['--train-dir', str(train), '--run-name', 'run', '--device', dev, '--beam-width', '16']
  run = lambda args: subprocess.run([sys.executable, os.path.join(ROOT, 'speecht-cli'), 'transcribe'] + base + args + [GOLDEN_FLAC],
                                    capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
  plain = run(['--output', str(tmp_path / 'plain.jsonl')])
  assert plain.returncode == 0, plain.stderr
  out = tmp_path / 'nbest.jsonl'
  got = run(['--nbest', '4', '--output', str(out)])
  assert got.returncode == 0, got.stderr
  lines, plain_lines = got.stdout.splitlines(), plain.stdout.splitlines()
  assert len(plain_lines) == 1 and lines[0] == plain_lines[0]
  rows = [l.split('\t') for l in lines[1:]]
  assert 1 <= len(rows) <= 4 and [r[1] for r in rows] == [str(i + 1) for i in range(len(rows))]
  assert all(r[0] == GOLDEN_FLAC and len(r) == 4 for r in rows) and rows[0][3] == lines[0].split('\t')[1]
  assert [float(r[2]) for r in rows] == sorted((float(r[2]) for r in rows), reverse=True)
  rec, = [json.loads(l) for l in out.read_text().splitlines()]
  rec_plain, = [json.loads(l) for l in (tmp_path / 'plain.jsonl').read_text().splitlines()]
  assert 'nbest' not in rec_plain and {k: rec[k] for k in rec_plain} == rec_plain
  assert [h['text'] for h in rec['nbest']] == [r[3] for r in rows] and all(set(h) == {'text', 'log_prob', 'acoustic'} for h in rec['nbest'])
  # a second pass: the model parts appear, and the first line carries the rescored winner
  out2 = tmp_path / 'rescored.jsonl'
  got2 = run(['--nbest', '4', '--rescore-language-model', TINY, '--rescore-lm-weight', '1.5', '--output', str(out2)])
  assert got2.returncode == 0, got2.stderr
  rec2, = [json.loads(l) for l in out2.read_text().splitlines()]
  assert all(set(h) == {'text', 'log_prob', 'acoustic', 'lm_log10', 'words', 'valid_words'} for h in rec2['nbest'])
  assert rec2['text'] == rec2['nbest'][0]['text'] == got2.stdout.splitlines()[0].split('\t')[1]
  assert sorted(h['text'] for h in rec2['nbest']) == sorted(h['text'] for h in rec['nbest'])
