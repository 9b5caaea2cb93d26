"""Hotword biasing of both CTC beam searches on the GPU (st_ctc_beam_search_decode_bias_nbest / _lm_bias_nbest: the BIAS
instantiations of ctc_beam_kernel) against the float64 specification of tests/hotword_oracle.py, bit identity with the unbiased
entry points where the bias is nothing, the behaviour the feature is for, the buffer discipline of the N-best entry points, and
the layers above -- transcribe, the CLI.

The comparison with the oracle is that of tests/test_gpu_nbest.py (nbest_oracle.check_list, rtol = atol = tau = 1e-4);
tests/test_hotwords_cpu.py shows on the oracle alone that near ties are rare in these cases and that the sets do not change when the
oracle runs in float32."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import hotword_oracle as H
from tests import lm_oracle as L
from tests import test_hotwords_cpu as HC
from tests import test_nbest_cpu as C
from tests.test_lm_oracle_cpu import word_logits

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests.test_gpu_nbest import _check, _engine  # noqa: E402  (after the importorskip, as that module does its own)

ROOT = C.ROOT
TINY = C.TINY
GOLDEN_FLAC = os.path.join(ROOT, 'tests', 'golden', '1089-134686-0037.flac')


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def _hotwords(phrases, weight=1.0):
  from speecht_amd.hotwords import Hotwords
  return Hotwords(phrases, weight)


# ---- oracle parity -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind,case,n', [(k, c, n) for k, c in HC.ALL_CASES for n in C.n_bests(c[0])])
def test_biased_lists_match_the_oracle(dev, tmp_path_factory, kind, case, n):
  from speecht_amd._lib import launch_trace
  beam, order, transform, phrases, weight, (logits, lens) = HC.case_parts(kind, case)
  eng = _engine(dev, logits, lens)
  hw = _hotwords(phrases, weight)
  with launch_trace() as tr:
    if kind == 'lm':
      lists = eng.lm_beam_search_decode_nbest(C.library_model(tmp_path_factory, order), n, beam, transform, hotwords=hw)
    else:
      lists = eng.beam_search_decode_nbest(n, beam, transform, hotwords=hw)
  name = '{}<{}>'.format('ctc_beam_lm_bias' if kind == 'lm' else 'ctc_beam_bias', 'wide' if beam > 64 else 'wave')
  assert any(l.startswith(name) and 'states={}'.format(hw.n_states) in l and l.endswith('nbest={}'.format(n)) for l in tr.lines), tr.lines
  sets = HC.oracle_sets(kind, case)
  assert [len(l) for l in lists] == [min(n, len(e)) for e in sets]
  assert len(lists[3]) == 1 and lists[3][0][0] == [] and len(lists[4]) == min(n, beam, 29)
  _check(lists, sets, n)


# ---- bit identity --------------------------------------------------------------------------------------------------------------------

def _bits(lists):
  return [[(ids, np.float32(s).view(np.int32).item()) for ids, s in hyps] for hyps in lists]


@pytest.mark.parametrize('beam', [16, 100, 128])
def test_no_bias_returns_the_bits_of_the_unbiased_entry_points(dev, beam):
  from speecht_amd._lib import launch_trace
  from speecht_amd.language_model import LanguageModel
  logits, lens = C.gpu_case(beam + 3)
  eng = _engine(dev, logits, lens)
  lm = LanguageModel.load(TINY)
  phrases = HC.PHRASE_SETS['cat']
  for transform in (None, 'log10_softmax'):
    free = lambda **kw: _bits(eng.beam_search_decode_nbest(beam, beam, transform, **kw))
    scored = lambda **kw: _bits(eng.lm_beam_search_decode_nbest(lm, beam, beam, transform, **kw))
    for search in (free, scored):
      before = search()
      with launch_trace() as tr:
        assert search(hotwords=_hotwords([])) == before                        # one state, no phrase
        assert search(hotwords=_hotwords(phrases, 0.0)) == before              # the whole automaton, every gain +-0
      assert sum('_bias<' in l for l in tr.lines) == 2, tr.lines
      biased = search(hotwords=_hotwords(phrases, 2.0))
      assert biased != before
      assert search() == before                                               # ... and a biased call leaves nothing behind


# ---- behaviour -----------------------------------------------------------------------------------------------------------------------

def _near_call():
  """Logits that spell 'the kat' with 'c' half a nat behind 'k' on the frames of the k (test_the_language_model_decides_the_spelling)
  and, as a second utterance, 'on the mat'."""
  rng = np.random.default_rng(7)
  x = word_logits('the kat', rng, noise=0.3)
  k, c = L.LETTERS.index('k'), L.LETTERS.index('c')
  for t in range(len(x)):
    if x[t].argmax() == k:
      x[t, c] = x[t, k] - 0.5
  y = word_logits('on the mat', rng, noise=0.3)
  T = max(len(x), len(y))
  logits = np.zeros((T, 2, 29), np.float32)
  logits[:len(x), 0], logits[:len(y), 1] = x, y
  return logits, [len(x), len(y)]


def test_hotwords_decide_a_near_call(dev):
  from speecht_amd.language_model import LanguageModel
  logits, lens = _near_call()
  eng = _engine(dev, logits, lens)
  lm = LanguageModel.load(TINY)
  searches = (lambda **kw: eng.beam_search_decode_nbest(1, 16, **kw),
              lambda **kw: eng.lm_beam_search_decode_nbest(lm, 1, 16, None, lm_weight=0.0, valid_word_count_weight=0.0, **kw))
  for search in searches:
    texts = lambda **kw: [L.ids_to_text(l[0][0]) for l in search(**kw)]
    plain = texts()
    assert plain == ['the kat', 'on the mat']
    # a hotword flips the transcript to the phrase (0.3 per character: 2.1 for 'the cat', more than the k's lead of 1.5)
    assert texts(hotwords=_hotwords(['the cat'], 0.3)) == ['the cat', 'on the mat']
    assert texts(hotwords=_hotwords([' cat', 'zebra'], 0.6)) == ['the cat', 'on the mat']
    # one that is only partially matched at the end does not: 'the cat' is lent 2.4 while it lasts, and the credit is returned
    assert texts(hotwords=_hotwords([' cats', ' cattle'], 0.6)) == plain
    assert texts(hotwords=_hotwords([' catalog'], 0.6)) == plain
    # a phrase absent from the audio leaves every transcript unchanged
    assert texts(hotwords=_hotwords(['zebra', 'quiz show'], 0.6)) == plain
  # the scores: the winner carries the banked credit, a partial match none, and the oracle agrees
  for phrases, weight, first in ((['the cat'], 0.3, 'the cat'), ([' cats', ' cattle'], 0.6, 'the kat')):
    hw = _hotwords(phrases, weight)
    lists = eng.beam_search_decode_nbest(16, 16, hotwords=hw)
    _check(lists, H.final_sets(logits.astype(np.float64), lens, 16, hotwords=phrases, hotword_weight=weight), 16)
    assert L.ids_to_text(lists[0][0][0]) == first
    cat = [ids for ids, _ in lists[0] if L.ids_to_text(ids) == 'the cat']
    assert len(cat) == 1 and hw.score(cat[0]) == pytest.approx((2.1, 2.1) if first == 'the cat' else (2.4, 0.0), abs=1e-12)


# ---- buffer discipline ------------------------------------------------------------------------------------------------------------------

def _raw_bias(eng, dev, beam, n, max_out, hw, lm=None, tables=None):
  """The biased entry points themselves with a `max_out` of the caller's over buffers filled with a pattern (test_gpu_nbest._raw_nbest);
  `tables`: a function that may spoil the st_bias_tables struct."""
  from speecht_amd import _lib
  lib = _lib.load()
  B = eng.dec_lens.numel()
  ws = torch.empty(lib.st_ctc_beam_ws(B, eng.t_out, beam) // 4 + 16, dtype=torch.int32, device=dev)
  ids = torch.full((B, n, max_out), -7, dtype=torch.int32, device=dev)
  lens = torch.full((B, n), -7, dtype=torch.int32, device=dev)
  logp = torch.full((B, n), 7.0, dtype=torch.float32, device=dev)
  count = torch.full((B,), -7, dtype=torch.int32, device=dev)
  nxt, gain, fin = hw.device_tables(dev)
  struct = _lib.BiasTables(nxt.data_ptr(), gain.data_ptr(), fin.data_ptr(), hw.n_states)
  bias = ctypes.byref(struct)
  if tables is not None:
    bias = tables(struct)
  eng._wait_uploads()
  torch.cuda.synchronize()
  tail = (eng._ptr(ids), max_out, eng._ptr(lens), eng._ptr(logp), eng._ptr(count), eng._ptr(ws), ws.numel() * 4, eng.stream_ptr)
  if lm is None:
    _lib.call('st_ctc_beam_search_decode_bias_nbest', eng.X[-1].ref, eng._ptr(eng.ctc_lens), beam, 0, bias, n, *tail)
  else:
    _lib.call('st_ctc_beam_search_decode_lm_bias_nbest', eng.X[-1].ref, eng._ptr(eng.ctc_lens), beam, 1, lm.device_handle(dev),
              ctypes.c_float(0.8), ctypes.c_float(0.0), ctypes.c_float(2.3), ctypes.c_float(-1000.0), bias, n, *tail)
  torch.cuda.synchronize()
  return ids.cpu().numpy(), lens.cpu().numpy(), logp.cpu().numpy(), count.cpu().numpy()


@pytest.mark.parametrize('with_lm', [False, True])
def test_truncated_labels_unused_slots_and_refused_arguments(dev, with_lm):
  from speecht_amd import _lib
  from speecht_amd.language_model import LanguageModel
  lm = LanguageModel.load(TINY) if with_lm else None
  logits, lens = C.gpu_case(77)
  eng = _engine(dev, logits, lens)
  hw = _hotwords(HC.PHRASE_SETS['on'], 1.0)
  beam, n = 100, 70                                          # two rounds of chain walks
  full = _raw_bias(eng, dev, beam, n, eng.t_out, hw, lm)
  cut = _raw_bias(eng, dev, beam, n, 3, hw, lm)
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
    assert all(a >= c for a, c in zip(full[2][b, :full[3][b]], full[2][b, 1:full[3][b]]))
  # refused arguments are errors, not launches
  def spoiled(**fields):
    def make(struct):
      for k, v in fields.items():
        setattr(struct, k, v)
      return ctypes.byref(struct)
    return make

  with _lib.launch_trace() as tr:
    for bad in (0, beam + 1):
      with pytest.raises(_lib.SpeechtHipError, match='n_best'):
        _raw_bias(eng, dev, beam, bad, 3, hw, lm)
    with pytest.raises(_lib.SpeechtHipError, match='null argument'):
      _raw_bias(eng, dev, beam, 2, 3, hw, lm, tables=lambda struct: None)
    for field in ('next', 'gain', 'fin'):
      with pytest.raises(_lib.SpeechtHipError, match='null hotword tables'):
        _raw_bias(eng, dev, beam, 2, 3, hw, lm, tables=spoiled(**{field: None}))
    for states in (0, -1, (1 << 20) + 1):
      with pytest.raises(_lib.SpeechtHipError, match='states supported'):
        _raw_bias(eng, dev, beam, 2, 3, hw, lm, tables=spoiled(n_states=states))
  assert tr.lines == []
  with pytest.raises(ValueError, match='n_best'):
    eng.beam_search_decode_nbest(17, 16, hotwords=hw)


# ---- the layers above -----------------------------------------------------------------------------------------------------------------

def test_transcribe_with_hotwords_is_the_engine_call(dev):
  from speecht_amd.engine import Wav2LetterEngine
  from speecht_amd.inference import transcribe
  from tests import workloads as WL
  layers = WL.w2l_layers(16, width=40, fc=72)
  params = WL.xavier_params(layers, seed=21, bias_range=0.3)
  params[-1] = (params[-1][0] * 12.0, params[-1][1] * 4.0)
  rng = np.random.default_rng(8)
  lengths = rng.integers(60, 260, 6).tolist()
  feats = [WL.synthetic_features(300 + i, t, 16).astype(np.float32) for i, t in enumerate(lengths)]
  eng = Wav2LetterEngine(layers, device=dev)
  eng.set_weights(params)
  opts = dict(lm_weight=2.0, valid_word_count_weight=1.0)
  plain_ids, plain_texts = transcribe(eng, feats, batch_size=8, beam_width=16)
  # phrases taken from what this random network says, so that the bias has something to hold on to
  phrases = sorted({t[i:i + 3] for t in plain_texts for i in range(0, max(len(t) - 2, 0), 5)})[:20] + ['zebra']
  hw = _hotwords(phrases, 1.5)
  key = lambda lists: sorted((tuple(h[0]), np.float32(h[1]).item()) for hyps in lists for h in hyps[:1])
  # no beam search asked for: beam 16; one batch, so the engine still holds the logits afterwards
  ids, texts = transcribe(eng, feats, batch_size=8, hotwords=hw)
  want = eng.beam_search_decode_nbest(1, 16, hotwords=hw)
  assert sorted(map(tuple, ids)) == sorted(tuple(l[0][0]) for l in want) and texts == [L.ids_to_text(i) for i in ids]
  assert len(ids) == len(plain_ids) and sum(hw.score(i)[1] for i in ids) > 0
  assert transcribe(eng, feats, batch_size=8, hotwords=phrases, beam_width=16)[0] == transcribe(eng, feats, batch_size=8, hotwords=_hotwords(phrases))[0]
  for decode in (dict(beam_width=32), dict(beam_width=32, language_model=TINY, lm_options=opts)):
    ids, texts, lists = transcribe(eng, feats, batch_size=8, nbest=4, hotwords=hw, timestamps=False, **decode)
    if 'language_model' in decode:
      from speecht_amd.language_model import LanguageModel
      want = eng.lm_beam_search_decode_nbest(LanguageModel.load(TINY), 4, 32, hotwords=hw, **opts)
    else:
      want = eng.beam_search_decode_nbest(4, 32, hotwords=hw)
    got = [[(h['ids'], h['log_prob']) for h in hyps] for hyps in lists]
    assert sorted(map(repr, got)) == sorted(map(repr, want))
    for i, hyps in enumerate(lists):
      assert hyps[0]['ids'] == ids[i] and hyps[0]['text'] == texts[i]
      for h in hyps:
        assert h['bias'] == hw.score(h['ids'])[1] and ('lm_log10' in h) == ('language_model' in decode)
        lm_part = opts['lm_weight'] * (h['lm_log10'] + opts['valid_word_count_weight'] * h['valid_words']) if 'lm_log10' in h else 0.0
        assert h['log_prob'] == pytest.approx(h['acoustic'] + lm_part + h['bias'], abs=1e-9)
  # spans and confidences belong to the biased text
  res = transcribe(eng, feats, batch_size=8, beam_width=16, hotwords=hw, timestamps=True, confidence=True)
  assert len(res) == 4 and all(res[2][i] is None or len(res[2][i]) == len(res[0][i]) for i in range(len(feats)))


def test_command_line_with_hotwords(dev, tmp_path):
  from speecht_amd import transcription
  from speecht_amd.speech_model import Session
  from tests.test_gpu_confidence import _golden_model
  model = _golden_model(tmp_path)
  train = tmp_path / 'train'
  (train / 'run').mkdir(parents=True)
  with Session(dev) as sess:
    model.init_session(sess)
    model.saver.save(sess, str(train / 'run' / 'speechT'), global_step=model.global_step)
    plain = transcription.transcribe_files(model.engine, [GOLDEN_FLAC], beam_width=16, nbest=4)[0]
    # a phrase the unbiased search ranks second if it has one, so that the bias can change the winner
    text = plain['nbest'][min(1, len(plain['nbest']) - 1)]['text'].strip()
    phrases = [text[:12].strip() or 'the', 'zebra']
    hw = _hotwords(phrases, 2.0)
    res = transcription.transcribe_files(model.engine, [GOLDEN_FLAC], beam_width=16, nbest=4, hotwords=hw)[0]
    want = model.engine.beam_search_decode_nbest(4, 16, hotwords=hw)[0]
  assert res['error'] is None and [(h['ids'], h['log_prob']) for h in res['nbest']] == want and res['ids'] == want[0][0]
  assert all(h['bias'] == hw.score(h['ids'])[1] for h in res['nbest'])
  words = tmp_path / 'words.txt'
  words.write_text('# hotwords\n{}\n'.format(phrases[0]))
  out = tmp_path / 'hot.jsonl'
  base = ['--train-dir', str(train), '--run-name', 'run', '--device', dev, '--beam-width', '16']
  got = subprocess.run([sys.executable, os.path.join(ROOT, 'speecht-cli'), 'transcribe'] + base +
                       ['--hotwords', str(words), '--hotword', 'zebra', '--hotword-weight', '2.0', '--nbest', '4', '--output', str(out),
                        GOLDEN_FLAC], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
  assert got.returncode == 0, got.stderr
  assert got.stdout.splitlines()[0] == '{}\t{}'.format(GOLDEN_FLAC, res['text'])
  rec, = [json.loads(l) for l in out.read_text().splitlines()]
  assert rec['text'] == res['text'] and [h['text'] for h in rec['nbest']] == [h['text'] for h in res['nbest']]
  assert all(set(h) == {'text', 'log_prob', 'acoustic', 'bias'} for h in rec['nbest'])
  assert [h['bias'] for h in rec['nbest']] == [h['bias'] for h in res['nbest']]
  assert [h['log_prob'] for h in rec['nbest']] == [h['log_prob'] for h in res['nbest']]
