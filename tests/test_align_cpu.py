"""Forced alignment without a GPU: the float64 oracle against brute force, the host form of the kernel (st_ctc_align_host, the
recursion the device shares through csrc/ctc_align_core.h) against the oracle, planted paths, the word / time / transcript
helpers, the CLI surface and the argument validation of the C ABI.

Accuracy condition (S* = oracle score, P = path under test, T = its frames):
    S* - path_score64(P)       <= 2 T 2^-24 |S*|
    |score - path_score64(P)|  <= T 2^-24 |S*| + 2^-23 |S*|
It bounds a lattice that rounds one fp32 sum per frame.  Measured on the inputs of this file (600 random + 120 planted cases,
T <= 200) and on the inputs of tests/test_gpu_align.py (T up to 1 501, labels up to 511), largest ratio of left side to bound:
    oracle recursion in numpy float32:            path 1.2e-3, score 0.31
    host form (double lattice, float score out):  path 1.8e-10, score 0.28
so fp32 would stay inside; the kernel keeps the lattice in double anyway (the device and the host form then agree bit for bit
and the path is the float64 optimum), and what remains of the score error is the rounding of the returned float.
"""
import ctypes
import importlib.machinery
import importlib.util
import itertools
import os

import numpy as np
import pytest

from tests import align_oracle as AO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_FLAC = os.path.join(ROOT, 'tests', 'golden', '1089-134686-0037.flac')
GOLDEN_TRANS = os.path.join(ROOT, 'tests', 'golden', '1089-134686.trans.txt')
ST_EINVAL = -1


def _cli():
  loader = importlib.machinery.SourceFileLoader('speecht_cli_align', os.path.join(ROOT, 'speecht-cli'))
  spec = importlib.util.spec_from_loader('speecht_cli_align', loader)
  cli = importlib.util.module_from_spec(spec)
  loader.exec_module(cli)
  return cli


def _p(a):
  return ctypes.c_void_p(a.ctypes.data)


def host_align(logits, labels, seq_lens, max_label_len=None):
  """st_ctc_align_host on a dense [B, T, C] batch -> (spans list, states [B, T], score [B], status [B])."""
  from speecht_amd import _lib
  lib = _lib.load()
  logits = np.ascontiguousarray(logits, dtype=np.float32)
  B, T, C = logits.shape
  lens = [len(l) for l in labels]
  offs = np.zeros(B + 1, dtype=np.int32)
  offs[1:] = np.cumsum(lens)
  ids = np.array([i for l in labels for i in l] + [0], dtype=np.int32)
  max_len = max(lens + [0]) if max_label_len is None else max_label_len
  spans = np.full((int(offs[-1]) + 1, 2), -7, dtype=np.int32)
  states = np.full((B, T), -7, dtype=np.int32)
  score = np.zeros(B, dtype=np.float32)
  status = np.full(B, -7, dtype=np.int32)
  ws = np.zeros(lib.st_ctc_align_ws(B, T, max_len) // 8 + 1, dtype=np.float64)
  _lib.call('st_ctc_align_host', _p(logits), B, T, C, _p(ids), _p(offs), _p(np.asarray(seq_lens, dtype=np.int32)), max_len,
            _p(spans), _p(states), _p(score), _p(status), _p(ws), ws.nbytes)
  assert (spans[-1] == -7).all()                       # nothing written past the last label
  return [spans[offs[b]:offs[b + 1]] for b in range(B)], states, score, status


def check_against_oracle(x, labels, spans, states, score, status, frames):
  """One utterance of a batch result against the oracle; returns the accuracy ratios (0, 0 for a label that does not fit)."""
  T = x.shape[0]
  ref = AO.align64(x, labels)
  assert (states[T:frames] == -2).all()
  if ref is None:
    assert status != 0 and score == -np.inf and (spans == -1).all() and (states[:T] == -2).all()
    return 0.0, 0.0
  assert status == 0
  st = states[:T]
  assert AO.is_valid_alignment(st, labels), (labels, st)
  assert (spans == AO.spans_from_states(st, len(labels))).all()
  assert (spans[:, 0] < spans[:, 1]).all() and (spans[1:, 0] >= spans[:-1, 1]).all()
  r = AO.accuracy_ratios(x, labels, st, float(score), ref[2])
  assert r[0] <= 1.0 and r[1] <= 1.0, r
  return r


def random_batches(seed, batches=75, batch=8):
  """600 utterances: T <= 200, L <= 60, 2..32 classes, ragged lengths, repeats, some labels that do not fit, some empty."""
  rng = np.random.default_rng(seed)
  for _ in range(batches):
    C = int(rng.choice([2, 3, 4, 5, 17, 29, 32]))
    xs, labs = [], []
    for _ in range(batch):
      T = int(rng.integers(0, 201))
      kind = rng.random()
      if kind < 0.1:
        L = 0
      elif kind < 0.25:
        L = int(rng.integers(max(T // 2, 0), T + 3)) if T else int(rng.integers(0, 3))     # around the edge of fitting
      else:
        L = int(rng.integers(0, min(T, 60) + 1))
      L = min(L, 60)
      labs.append(AO.random_labels(rng, L, C))
      xs.append(AO.random_logits(rng, T, C, scale=float(rng.choice([0.05, 1.0, 3.0, 10.0]))))
    yield xs, labs


def planted_batches(seed, batches=15, batch=8):
  rng = np.random.default_rng(seed)
  for _ in range(batches):
    C = int(rng.choice([3, 5, 29, 32]))
    xs, labs, paths = [], [], []
    for _ in range(batch):
      L = int(rng.integers(0, 61))
      lab = AO.random_labels(rng, L, C)
      T = int(rng.integers(max(AO.min_frames(lab), 1), 201))
      x, path = AO.planted_logits(rng, lab, T, C)
      xs.append(x)
      labs.append(lab)
      paths.append(path)
    yield xs, labs, paths


# ---- the oracle ---------------------------------------------------------------------------------------------------------------

def test_oracle_matches_brute_force():
  """Every per-frame class sequence of C = 4 classes over T <= 7 frames that collapses to the label is an alignment: the oracle
  returns the best of them, with its score."""
  rng = np.random.default_rng(5)
  C, blank = 4, 3
  label_sets = [[]] + [list(l) for n in (1, 2, 3) for l in itertools.product(range(3), repeat=n)]
  checked = 0
  for T in range(0, 8):
    seqs = list(itertools.product(range(C), repeat=T))
    collapsed = [AO.states_from_classes(s, blank) for s in seqs]
    for labels in label_sets:
      x = AO.random_logits(rng, T, C, scale=2.0)
      ly = AO.log_softmax64(x)
      best, best_states = None, None
      for s, (states, lab) in zip(seqs, collapsed):
        if lab == labels:
          sc = float(ly[np.arange(T), list(s)].sum()) if T else 0.0
          if best is None or sc > best:
            best, best_states = sc, states
      ref = AO.align64(x, labels)
      if best is None:
        assert ref is None and T < AO.min_frames(labels)
        continue
      assert ref is not None and T >= AO.min_frames(labels)
      assert list(ref[0]) == best_states, (T, labels)
      assert abs(ref[2] - best) <= 1e-12 * max(1.0, abs(best))
      assert AO.is_valid_alignment(ref[0], labels)
      assert abs(AO.path_score64(x, ref[0], labels) - best) <= 1e-12 * max(1.0, abs(best))
      checked += 1
  assert checked > 150


def test_oracle_tie_rules():
  """Uniform logits: every path ties.  Stay wins over advance, so the path enters as late as the end rule allows and the
  end tie goes to the last label state."""
  x = np.zeros((3, 4), dtype=np.float32)
  states, spans, score = AO.align64(x, [1])
  assert list(states) == [0, 0, 0] and spans.tolist() == [[0, 3]]
  assert abs(score - 3 * np.log(0.25)) < 1e-12
  states, spans, _ = AO.align64(np.zeros((5, 4), dtype=np.float32), [0, 1])
  # end: label 1; back-pointers prefer stay, then advance (from the blank between), then skip
  assert AO.is_valid_alignment(states, [0, 1]) and states[-1] == 1
  assert list(states) == [0, 1, 1, 1, 1]
  states, spans, score = AO.align64(np.zeros((4, 3), dtype=np.float32), [])
  assert list(states) == [-1] * 4 and spans.shape == (0, 2)


# ---- the host form ------------------------------------------------------------------------------------------------------------

def test_library_exports_the_aligner():
  from speecht_amd import _lib
  lib = _lib.load()
  for name in ('st_ctc_align_ws', 'st_ctc_align_f32', 'st_ctc_align_host'):
    assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS


def test_host_form_against_oracle_random():
  worst = [0.0, 0.0]
  n = bad = 0
  for xs, labs in random_batches(11):
    logits, lens = AO.pad_batch(xs)
    spans, states, score, status = host_align(logits, labs, lens)
    for b, (x, lab) in enumerate(zip(xs, labs)):
      r = check_against_oracle(x, lab, spans[b], states[b], score[b], status[b], logits.shape[1])
      assert (status[b] != 0) == (x.shape[0] < AO.min_frames(lab))
      worst = [max(worst[0], r[0]), max(worst[1], r[1])]
      n += 1
      bad += int(status[b] != 0)
  print('host form, random cases: {} utterances ({} do not fit), largest ratio to the bound: path {:.3g}, score {:.3g}'.format(
      n, bad, *worst))
  assert n >= 300 and 10 <= bad < n // 2


def test_host_form_ties_as_the_oracle():
  """All-equal logits (every comparison ties) and logits from a two-value set (many ties): identical paths."""
  rng = np.random.default_rng(3)
  for _ in range(40):
    C = int(rng.choice([2, 4, 29]))
    T = int(rng.integers(1, 60))
    lab = AO.random_labels(rng, int(rng.integers(0, T // 2 + 1)), C)
    for x in (np.zeros((T, C), dtype=np.float32), rng.integers(0, 2, (T, C)).astype(np.float32)):
      ref = AO.align64(x, lab)
      spans, states, score, status = host_align(x[None], [lab], [T])
      if ref is None:
        assert status[0] != 0
        continue
      assert status[0] == 0 and list(states[0]) == list(ref[0]) and (spans[0] == ref[1]).all()


def test_host_form_planted_paths():
  n = 0
  for xs, labs, paths in planted_batches(21):
    logits, lens = AO.pad_batch(xs)
    spans, states, score, status = host_align(logits, labs, lens)
    for b, (x, lab, path) in enumerate(zip(xs, labs, paths)):
      planted = [u // 2 if u & 1 else -1 for u in path]
      ref = AO.align64(x, lab)
      assert list(ref[0]) == planted                          # first: the oracle finds the planted path
      assert status[b] == 0 and list(states[b, :len(planted)]) == planted
      assert (spans[b] == ref[1]).all()
      check_against_oracle(x, lab, spans[b], states[b], score[b], status[b], logits.shape[1])
      n += 1
  assert n == 120


def test_host_form_one_bad_utterance_leaves_its_neighbours_alone():
  rng = np.random.default_rng(8)
  C = 29
  labs = [AO.random_labels(rng, 40, C, 0.1), AO.random_labels(rng, 30, C), AO.random_labels(rng, 10, C)]
  xs = [AO.random_logits(rng, 80, C), AO.random_logits(rng, 25, C), AO.random_logits(rng, 60, C)]
  logits, lens = AO.pad_batch(xs)
  spans, states, score, status = host_align(logits, labs, lens)
  assert status.tolist() == [0, 1, 0] and (spans[1] == -1).all()
  for b in (0, 2):
    s1, st1, sc1, stat1 = host_align(logits[b:b + 1], [labs[b]], lens[b:b + 1])
    assert (s1[0] == spans[b]).all() and (st1[0] == states[b]).all() and sc1[0] == score[b]
  # a label longer than the dispatch was made for (max_label_len 12: up to 31 labels) is refused per utterance
  _, _, sc, stat = host_align(logits, labs, lens, max_label_len=12)
  assert stat.tolist() == [1, 1, 0] and sc[0] == -np.inf
  # states may be left out
  from speecht_amd import _lib
  lib = _lib.load()
  offs = np.array([0, 40, 70, 80], dtype=np.int32)
  ids = np.array(sum(labs, []), dtype=np.int32)
  sp = np.zeros((80, 2), dtype=np.int32)
  sc2, stat2 = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.int32)
  ws = np.zeros(lib.st_ctc_align_ws(3, 80, 40) // 8 + 1, dtype=np.float64)
  _lib.call('st_ctc_align_host', _p(logits), 3, 80, C, _p(ids), _p(offs), _p(lens), 40, _p(sp), None, _p(sc2), _p(stat2), _p(ws),
            ws.nbytes)
  assert (sp[:40] == spans[0]).all() and (sc2 == score).all()


def test_abi_argument_validation():
  from speecht_amd import _lib
  from speecht_amd._lib import Tensor3
  lib = _lib.load()
  B, T, C = 2, 10, 5
  for L in (0, 1, 31, 32, 300, 511):
    assert lib.st_ctc_align_ws(B, T, L) == B * T * (32 * 8 + 64 * 4) + B * 4 + 512
  assert lib.st_ctc_align_ws(B, T, 512) == 0 and lib.st_ctc_align_ws(B, T, -1) == 0
  assert lib.st_ctc_align_ws(0, T, 3) == 0 and lib.st_ctc_align_ws(B, 0, 3) == 0
  x = np.zeros((B, T, 32), dtype=np.float32)
  ids, offs, lens = np.zeros(4, dtype=np.int32), np.array([0, 2, 4], dtype=np.int32), np.array([T, T], dtype=np.int32)
  spans, states = np.zeros((4, 2), dtype=np.int32), np.zeros((B, T), dtype=np.int32)
  score, status = np.zeros(B, dtype=np.float32), np.zeros(B, dtype=np.int32)
  need = lib.st_ctc_align_ws(B, T, 2)
  ws = np.zeros(need // 8 + 1, dtype=np.float64)

  def host(**kw):
    a = dict(logits=_p(x), C=C, ids=_p(ids), offs=_p(offs), lens=_p(lens), L=2, spans=_p(spans), states=_p(states),
             score=_p(score), status=_p(status), ws=_p(ws), nbytes=ws.nbytes)
    a.update(kw)
    return lib.st_ctc_align_host(a['logits'], B, T, a['C'], a['ids'], a['offs'], a['lens'], a['L'], a['spans'], a['states'],
                                 a['score'], a['status'], a['ws'], a['nbytes'])

  def device(desc=None, **kw):
    # every argument is refused before anything is launched: no device is touched
    d = desc if desc is not None else Tensor3(x.ctypes.data, B, T, C, 0, T, 32)
    a = dict(ids=_p(ids), offs=_p(offs), lens=_p(lens), L=2, spans=_p(spans), states=_p(states), score=_p(score),
             status=_p(status), ws=_p(ws), nbytes=ws.nbytes)
    a.update(kw)
    return lib.st_ctc_align_f32(ctypes.byref(d), a['ids'], a['offs'], a['lens'], a['L'], a['spans'], a['states'], a['score'],
                                a['status'], a['ws'], a['nbytes'], None)

  assert host() == 0
  for fn in (host, device):
    for name in ('ids', 'offs', 'lens', 'spans', 'score', 'status', 'ws'):
      assert fn(**{name: None}) == ST_EINVAL, (fn.__name__, name)
      assert b'null' in lib.st_last_error()
    assert fn(L=512) == ST_EINVAL and b'511' in lib.st_last_error()
    assert fn(L=-1) == ST_EINVAL
    assert fn(nbytes=need - 1) == ST_EINVAL and b'workspace' in lib.st_last_error()
  assert host(logits=None) == ST_EINVAL
  assert host(C=33) == ST_EINVAL and host(C=1) == ST_EINVAL
  assert lib.st_ctc_align_f32(None, _p(ids), _p(offs), _p(lens), 2, _p(spans), _p(states), _p(score), _p(status), _p(ws), ws.nbytes,
                              None) == ST_EINVAL
  assert device(desc=Tensor3(None, B, T, C, 0, T, 32)) == ST_EINVAL
  x64 = np.zeros((B, T, 64), dtype=np.float32)
  assert device(desc=Tensor3(x64.ctypes.data, B, T, 33, 0, T, 64)) == ST_EINVAL and b'num_classes' in lib.st_last_error()
  assert device(desc=Tensor3(x.ctypes.data, B, T, 1, 0, T, 32)) == ST_EINVAL


# ---- words, times, transcripts, CLI ---------------------------------------------------------------------------------------------

def _ids_spans(text):
  from speecht_amd import vocabulary
  ids = vocabulary.sentence_to_ids(text)
  return ids, [(2 * k, 2 * k + 1) for k in range(len(ids))]


def test_word_spans():
  from speecht_amd.alignment import char_spans, word_spans
  ids, spans = _ids_spans('the cat')
  assert word_spans(ids, spans) == [('the', 0, 5), ('cat', 8, 13)]
  ids, spans = _ids_spans('a  b')                                  # double space
  assert word_spans(ids, spans) == [('a', 0, 1), ('b', 6, 7)]
  ids, spans = _ids_spans('  hi there ')                           # leading and trailing space
  assert word_spans(ids, spans) == [('hi', 4, 7), ('there', 10, 19)]
  ids, spans = _ids_spans("don't stop")                            # the apostrophe is a letter of its word
  assert word_spans(ids, spans) == [("don't", 0, 9), ('stop', 12, 19)]
  assert word_spans([], []) == [] and word_spans(*_ids_spans('   ')) == []
  assert char_spans(*_ids_spans("a'")) == [('a', 0, 1), ("'", 2, 3)]
  spans = np.array([[3, 5], [5, 9]], dtype=np.int32)               # arrays as engine.align returns them
  assert word_spans([7, 8], spans) == [('hi', 3, 9)]


def test_frames_to_seconds():
  from speecht_amd.alignment import frames_to_seconds, timed_words
  assert frames_to_seconds(0, 22050) == 0.0
  assert frames_to_seconds(100, 16000) == 2.0                      # 100 * 320 / 16000
  assert abs(frames_to_seconds(501, 22050) - 501 * 320 / 22050) < 1e-12
  assert frames_to_seconds(10, 16000, hop_length=80) == 0.1
  assert frames_to_seconds(100, 16000, duration=1.5) == 1.5        # clipped to the file
  assert frames_to_seconds(10, 16000, duration=1.5) == 0.2
  ids, spans = _ids_spans('ab c')
  words = timed_words(ids, spans, 16000, duration=0.1)
  assert words == [dict(word='ab', start=0.0, end=0.06), dict(word='c', start=0.1, end=0.1)]
  chars = timed_words(ids, spans, 16000, chars=True)
  assert [c['char'] for c in chars] == ['a', 'b', ' ', 'c'] and chars[1] == dict(char='b', start=0.04, end=0.06)


def test_transcript_files(tmp_path):
  from speecht_amd import alignment, vocabulary
  from speecht_amd.transcription import TranscriptionError
  table = alignment.read_transcripts(GOLDEN_TRANS)
  text = table['1089-134686-0037']
  assert text == text.upper() and len(text.split()) > 3
  # ids exactly as the corpus reader makes them
  from speecht_amd.preprocessing import SpeechCorpusReader
  reader_ids = dict(SpeechCorpusReader(os.path.dirname(GOLDEN_TRANS))._transcript_dict)['1089-134686-0037']
  assert alignment.transcript_ids(text) == reader_ids == vocabulary.sentence_to_ids(text.lower())
  f = tmp_path / 'x.trans.txt'
  f.write_text("a-1 HELLO  WORLD\na-2  LEADING\nempty-id\n\nb-1 DON'T\n")
  t = alignment.read_transcripts(str(f))
  assert t == {'a-1': 'HELLO  WORLD', 'a-2': ' LEADING', 'empty-id': '', 'b-1': "DON'T"}
  assert alignment.transcript_ids('') == []
  assert alignment.transcript_ids("Don't") == [3, 14, 13, 26, 19]
  with pytest.raises(TranscriptionError):
    alignment.transcript_ids('route 66')
  # beside the audio file, or the file given
  audio = tmp_path / 'a-1.flac'
  other = tmp_path / 'zz.wav'
  found = alignment.find_transcripts([str(audio), str(other)])
  assert found == {str(audio): 'HELLO  WORLD', str(other): None}
  g = tmp_path / 'given.txt'
  g.write_text('zz OTHER\n')
  assert alignment.find_transcripts([str(audio), str(other)], str(g)) == {str(audio): None, str(other): 'OTHER'}
  assert alignment.find_transcripts([GOLDEN_FLAC])[GOLDEN_FLAC] == text


def test_cli_parsing():
  cli = _cli()
  _, flags = cli.parse(['align', 'a.flac'])
  assert (flags.command, flags.paths, flags.batch_size, flags.sample_rate) == ('align', ['a.flac'], 1, 22050)
  assert (flags.transcripts, flags.chars, flags.output, flags.feature_type) == (None, False, None, 'power')
  _, flags = cli.parse(['align', '--transcripts', 't.txt', '--chars', '--output', 'o.json', '--batch-size', '4', '--sample-rate',
                        'native', '--mfcc', '--run-name', 'r', 'd', 'b.wav'])
  assert (flags.transcripts, flags.chars, flags.output, flags.batch_size, flags.sample_rate, flags.feature_type, flags.paths) == \
      ('t.txt', True, 'o.json', 4, 'native', 'mfcc', ['d', 'b.wav'])
  assert flags.run_train_dir == 'train/r'
  with pytest.raises(SystemExit):
    cli.parse(['align'])                                           # PATH is required
  _, flags = cli.parse(['transcribe', 'a.flac'])
  assert flags.timestamps is False and flags.batch_size == 1
  _, flags = cli.parse(['transcribe', '--timestamps', '--beam-width', '16', 'a.flac'])
  assert flags.timestamps is True and flags.beam_width == 16
  _, flags = cli.parse(['train'])
  assert flags.batch_size == 64 and not hasattr(flags, 'timestamps')


def test_align_files_reports_problems_as_entries(tmp_path):
  """No transcript, an unreadable file, a transcript outside the vocabulary: error entries, not exceptions (and no device is
  needed when nothing is left to align)."""
  from speecht_amd.alignment import align_files
  missing = str(tmp_path / 'nothing.flac')
  res = align_files(None, [GOLDEN_FLAC, missing, GOLDEN_FLAC], [None, 'HELLO', 'ROUTE 66'])
  assert [r['path'] for r in res] == [GOLDEN_FLAC, missing, GOLDEN_FLAC]
  assert 'no transcript' in res[0]['error'] and res[0]['seconds'] > 1.0 and res[0]['spans'] is None
  assert 'no such file' in res[1]['error']
  assert 'outside the vocabulary' in res[2]['error']
  long = align_files(None, [GOLDEN_FLAC], {GOLDEN_FLAC: 'A' * 512})
  assert 'too long' in long[0]['error']
