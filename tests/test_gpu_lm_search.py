"""The LM weight search on the GPU: the multi-candidate LM beam search (st_ctc_beam_search_decode_lm_candidates) against single
searches bit for bit, the batched edit-distance kernel (st_edit_distance_pairs) against editdistance.eval, the device scorer
against the host path and run_step, and `speecht-cli search` end to end against single-candidate decodes + run_step."""
import contextlib
import io
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import lm_oracle as L
from tests.test_gpu_lm_beam import SENTENCE_WORDS, _cases, _engine
from tests.test_lm_search_cpu import _fields, _run_step_stats, _sparse

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, 'tests', 'golden', 'lm_tiny.arpa')
_MODELS = {}


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def _model(tmp_dir, order):
  from speecht_amd.language_model import LanguageModel
  if order == 3:
    return LanguageModel.load(TINY)
  if order not in _MODELS:
    text = L.random_arpa(200 + order, 150, [400, 300, 200, 100][:order - 1], extra_words=SENTENCE_WORDS)
    path = os.path.join(tmp_dir, 's{}.arpa'.format(order))
    with open(path, 'w') as f:
      f.write(text)
    _MODELS[order] = LanguageModel.load(path)
  return _MODELS[order]


def _weights(P, seed):
  rng = np.random.default_rng(seed)
  w = np.column_stack([rng.uniform(0.0, 3.0, P), rng.uniform(-2.0, 2.0, P), rng.uniform(0.0, 4.0, P)]).astype(np.float32)
  w[P // 2] = 0.0                                            # a candidate with every weight 0
  return w


@pytest.mark.parametrize('beam', [1, 16, 64, 100, 128])
@pytest.mark.parametrize('order', [1, 3, 5])
def test_candidates_equal_single_searches_bit_for_bit(dev, tmp_path_factory, beam, order):
  lm = _model(str(tmp_path_factory.getbasetemp()), order)
  logits, lens = _cases(7 * beam + order)                   # lengths 80, .., 77, 0, 1
  eng = _engine(dev, logits, lens)
  P = [1, 3, 17][(beam + order) % 3]
  w = _weights(P, beam + 100 * order)
  for transform in (None, 'log10_softmax'):
    got = eng.lm_beam_search_decode_candidates(lm, w, beam, transform)
    ids, olens, olp = got.ids.cpu().numpy(), got.lens.cpu().numpy(), got.log_prob.cpu().numpy()
    host = got.host()
    for p in range(P):
      s_ids, s_lp = eng.lm_beam_search_decode(lm, beam, transform, lm_weight=float(w[p, 0]), word_count_weight=float(w[p, 1]),
                                              valid_word_count_weight=float(w[p, 2]))
      s_lens = eng.dec_lens.cpu().numpy()
      s_raw = eng.dec_ids.view(-1, eng.t_out).cpu().numpy()
      assert host[p][0] == s_ids
      assert np.array_equal(olens[p], s_lens)
      assert np.array_equal(olp[p].view(np.uint32), s_lp.reshape(-1).view(np.uint32))
      for b in range(len(lens)):
        assert np.array_equal(ids[p, b, :olens[p, b]], s_raw[b, :s_lens[b]])
      if not w[p].any():
        f_ids, f_lp = eng.beam_search_decode(beam, transform)
        assert host[p][0] == f_ids and np.array_equal(host[p][1].view(np.uint32), f_lp.view(np.uint32))
    assert host[0][0][3] == []


def test_chunked_and_unchunked_candidate_runs_agree(dev):
  """Python chunks (a small workspace bound: one candidate per call) and the library's own split of more than 64 triples per
  launch give the outputs of one unsplit call."""
  from speecht_amd.language_model import LanguageModel
  lm = LanguageModel.load(TINY)
  logits, lens = _cases(77)
  eng = _engine(dev, logits, lens)
  w = _weights(70, 5)
  whole = eng.lm_beam_search_decode_candidates(lm, w, 16)
  a = [t.cpu().numpy().copy() for t in (whole.ids, whole.lens, whole.log_prob)]
  pieces = eng.lm_beam_search_decode_candidates(lm, w[:9], 16, max_workspace_bytes=1)
  b = [t.cpu().numpy() for t in (pieces.ids, pieces.lens, pieces.log_prob)]
  assert np.array_equal(a[0][:9], b[0]) and np.array_equal(a[1][:9], b[1]) and np.array_equal(a[2][:9].view(np.uint32), b[2].view(np.uint32))
  s_ids, s_lp = eng.lm_beam_search_decode(lm, 16, lm_weight=float(w[66, 0]), word_count_weight=float(w[66, 1]),
                                          valid_word_count_weight=float(w[66, 2]))
  assert whole.host()[66][0] == s_ids and np.array_equal(a[2][66].view(np.uint32), s_lp.reshape(-1).view(np.uint32))


def test_candidates_refuse_a_handle_without_a_copy_on_the_device(dev):
  import ctypes
  from speecht_amd import _lib
  from speecht_amd.language_model import LanguageModel
  lm = LanguageModel(TINY)                                  # a fresh handle, not uploaded anywhere
  logits, lens = _cases(3)
  eng = _engine(dev, logits, lens)
  lib = _lib.load()
  B = eng.dec_lens.numel()
  ws = torch.empty(lib.st_ctc_beam_lm_candidates_ws(B, eng.t_out, 16, 2) // 4 + 16, dtype=torch.int32, device=dev)
  out = torch.empty(2 * B * eng.t_out, dtype=torch.int32, device=dev)
  w = (ctypes.c_float * 6)(0.8, 0.0, 2.3, 1.0, 0.0, 0.0)
  eng._wait_uploads()
  with pytest.raises(_lib.SpeechtHipError, match='not on device'):
    _lib.call('st_ctc_beam_search_decode_lm_candidates', eng.X[-1].ref, eng._ptr(eng.ctc_lens), 16, 0, lm._handle, w, 2,
              ctypes.c_float(-1000.0), eng._ptr(out), eng.t_out, eng._ptr(out), eng._ptr(out), eng._ptr(ws), ws.numel() * 4,
              eng.stream_ptr)
  got = eng.lm_beam_search_decode_candidates(lm, [(0.8, 0.0, 2.3)], 16)     # the engine uploads to its own device first
  assert len(got.host()[0][0]) == B


def _device_distances(dev, expected, decoded, pairs):
  import ctypes
  from speecht_amd import _lib

  def mat(rows):
    pitch = max([len(r) for r in rows] + [1])
    m = np.zeros((len(rows), pitch), dtype=np.int32)
    for i, r in enumerate(rows):
      m[i, :len(r)] = r
    return torch.as_tensor(m).to(dev), torch.as_tensor(np.array([len(r) for r in rows], dtype=np.int32)).to(dev), pitch
  ea, el, ep = mat(expected)
  da, dl, dp = mat(decoded)
  pr = torch.as_tensor(np.asarray(pairs, dtype=np.int32)).to(dev)
  out = torch.full((len(pairs) * 2,), -7, dtype=torch.int32, device=dev)
  p = lambda t: ctypes.c_void_p(t.data_ptr())
  _lib.call('st_edit_distance_pairs', p(ea), len(expected), ep, p(el), p(da), len(decoded), dp, p(dl), p(pr), len(pairs), p(out),
            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
  return out.cpu().numpy().reshape(-1, 2)


def test_edit_distance_kernel_equals_editdistance_eval(dev):
  from speecht_amd import editdistance, vocabulary as V
  ids = V.sentence_to_ids
  rng = np.random.default_rng(2024)
  seqs = [[], ids(' '), ids('   '), ids(' a'), ids('a '), ids('  the  cat  '), ids("it's"), ids("its"), ids('the cat sat'),
          ids('the bat sat on it'), ids("don't  stop'"), ids('a b c d e f g'), ids('abcdefghijklmnopqrstuvwxyz')]
  for n in (1, 5, 63, 64, 65, 127, 128, 129, 180, 460):
    s = rng.integers(0, 28, n)
    s[rng.random(n) < 0.25] = 27
    seqs.append(s.tolist())
  # words drawn from a small set, so that equal words in different places are the common case
  vocab = ['the', 'cat', 'sat', 'on', 'a', "it's", 'mat', 'at', 'tea', 'eat']
  for n in (3, 40, 400):
    seqs.append(ids(' '.join(rng.choice(vocab, n))))
  long_words = ids(' '.join(rng.choice(vocab, 400)))
  seqs.append((long_words * 3)[:2000])
  pairs = [(i, j) for i in range(len(seqs)) for j in range(len(seqs)) if (i + j) % 3 == 0 or i == j or min(i, j) < 13]
  got = _device_distances(dev, seqs, seqs, pairs)
  for (i, j), (led, wed) in zip(pairs, got):
    a, b = V.ids_to_sentence(seqs[i]), V.ids_to_sentence(seqs[j])
    assert led == editdistance.eval(a, b), (i, j)
    assert wed == editdistance.eval(a.split(), b.split()), (i, j)
  # 2 000 letters against a different 2 000 letters
  x, y = (long_words * 3)[:2000], ids(' '.join(rng.choice(vocab, 500)))[:2000]
  (led, wed), = _device_distances(dev, [x], [y], [(0, 0)])
  assert led == editdistance.eval(V.ids_to_sentence(x), V.ids_to_sentence(y))
  assert wed == editdistance.eval(V.ids_to_sentence(x).split(), V.ids_to_sentence(y).split())
  # refused pairs: an id outside 0..27, a sequence longer than the kernel's bound, a row index out of range
  from speecht_amd import _lib
  too_long = [1] * (_lib.load().st_edit_distance_max_len() + 1)
  got = _device_distances(dev, [ids('ab'), [1, 28, 2], too_long], [ids('ab'), [-1]], [(0, 0), (1, 0), (0, 1), (2, 0), (0, 5)])
  assert got.tolist() == [[0, 0], [-1, -1], [-1, -1], [-1, -1], [-1, -1]]


@pytest.mark.parametrize('pair_by_row', [False, True])
def test_device_scorer_equals_the_host_path_and_run_step(dev, pair_by_row):
  from speecht_amd import vocabulary as V
  from speecht_amd.candidate_scoring import score_candidates
  from speecht_amd.language_model import LanguageModel
  lm = LanguageModel.load(TINY)
  logits = (np.random.default_rng(31).standard_normal((80, 5, 29)) * 2.0).astype(np.float32)
  lens = [0, 80, 40, 77, 30] if not pair_by_row else [80, 40, 0, 77, 30]      # an empty decoding (row 0: the walk survives it)
  eng = _engine(dev, logits, lens)
  labels = [V.sentence_to_ids(s) for s in ('the cat', "it's a  mat", 'on the mat ', ' a', 'dog')]
  w = _weights(6, 9)
  got = eng.lm_beam_search_decode_candidates(lm, w, 16, None)
  host_rows = [h[0] for h in got.host()]
  assert all(rows[0 if not pair_by_row else 2] == [] for rows in host_rows)
  dev_stats = score_candidates(_sparse(labels), got, pair_by_row=pair_by_row, device=True)
  host_stats = score_candidates(_sparse(labels), got, pair_by_row=pair_by_row, device=False)
  for p in range(len(w)):
    want = _run_step_stats(labels, host_rows[p], pair_by_row)
    assert _fields(dev_stats[p]) == _fields(host_stats[p]) == _fields(want), p


_LINE = re.compile(r'^-?\d+\.\d\d Candidate \(lm_weight=')


def test_cli_search_end_to_end(dev, tmp_path):
  """`speecht-cli search --max-iterations 6 --seed 1` with K = 1 and K = 3 on a 3-step checkpoint, a four-utterance dev set and
  lm_tiny.arpa prints candidate lines; the same seeded walk in-process, every candidate scored by a single-candidate search
  and run_step's own statistics on the same batches, prints the same lines."""
  from tests import workloads as WL  # noqa: F401
  from oracle import w2l_oracle as O
  from tests.test_gpu_api import write_wav
  data = tmp_path / 'data'
  texts = ['THE CAT SAT ON THE MAT', 'A DOG', "IT'S THE CAT", 'ON A MAT']
  for split in ('train', 'dev'):
    (data / split).mkdir(parents=True)
    lines = []
    for i in range(4):
      uid = 'spk-{}-{:04d}'.format(split, i)
      write_wav(str(data / split / (uid + '.wav')), O.synthetic_audio(i + (0 if split == 'train' else 10), 24000))
      lines.append('{} {}'.format(uid, texts[i]))
    (data / split / 'x.trans.txt').write_text('\n'.join(lines) + '\n')
  cli = [sys.executable, os.path.join(ROOT, 'speecht-cli')]
  common = ['--data-dir', str(data), '--train-dir', str(tmp_path / 'train'), '--log-dir', str(tmp_path / 'log'),
            '--run-name', 'ci', '--batch-size', '2']
  run = lambda args: subprocess.run(cli + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
  r = run(['preprocess'] + common)
  assert r.returncode == 0, r.stdout + r.stderr
  r = run(['train'] + common + ['--steps-per-checkpoint', '3', '--max-steps', '3', '--learning-rate', '1e-3'])
  assert r.returncode == 0, r.stdout + r.stderr

  from speecht_amd.evaluation import EvalStatistics, Evaluation
  from speecht_amd.parameter_search import LanguageModelParameterSearch
  from speecht_amd.speech_input import SparseTensorValue

  class SingleSearches(LanguageModelParameterSearch):
    def score_candidates(self, model, sess, candidates):
      label, = model.step(sess, loss=False, update=False, decode=False, return_label=True)
      for c in candidates:
        ids, _ = model.engine.lm_beam_search_decode(model.language_model, model.beam_width, model.beam_input,
                                                    lm_weight=c.lm_weight, word_count_weight=c.word_count_weight,
                                                    valid_word_count_weight=c.valid_word_count_weight)
        idx = [[b, p] for b, seq in enumerate(ids) for p in range(len(seq))]
        decoded = SparseTensorValue(np.array(idx, dtype=np.int64).reshape(-1, 2), np.array([v for s in ids for v in s], dtype=np.int64),
                                    np.array([len(ids), max([len(s) for s in ids] + [0])], dtype=np.int64))
        fake = types.SimpleNamespace(global_step=types.SimpleNamespace(eval=lambda: 0),
                                     step=lambda sess, **kw: [np.float32(0.0), [decoded], label])
        stats = EvalStatistics()
        Evaluation.run_step(self, fake, sess, stats, save=False, verbose=False)
        c.update_score(-(stats.global_letter_error_rate + stats.global_word_error_rate), stats)

  loader = __import__('importlib.machinery').machinery.SourceFileLoader('speecht_cli_e2e', os.path.join(ROOT, 'speecht-cli'))
  spec = __import__('importlib.util').util.spec_from_loader('speecht_cli_e2e', loader)
  cli_mod = __import__('importlib.util').util.module_from_spec(spec)
  loader.exec_module(cli_mod)
  for k in (1, 3):
    args = ['search', '--max-iterations', '6', '--seed', '1', '--candidates-per-batch', str(k), '--pair-by-row',
            '--language-model', TINY, '--population-size', '4'] + common
    r = run(args)
    assert r.returncode == 0, r.stdout + r.stderr
    printed = [l for l in r.stdout.splitlines() if _LINE.match(l)]
    assert len(printed) == 7 + 4, r.stdout                  # 1 + 6 new candidates, then the population of 4 best-first
    _, flags = cli_mod.parse(args)
    flags.run_train_dir = str(tmp_path / 'train' / 'ci')
    buf = io.StringIO()
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
      with contextlib.redirect_stdout(buf):
        SingleSearches(flags).run()
    finally:
      os.chdir(cwd)
    want = [l for l in buf.getvalue().splitlines() if _LINE.match(l)]
    assert printed == want, (k, printed, want)
