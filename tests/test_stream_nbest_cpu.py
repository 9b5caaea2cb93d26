"""N-best lists for the finals of live streams, the parts that need no GPU: the arena's parser on hand-made arrays (records in any
order, short lists, an empty hypothesis, an arena that was too small, records that cannot be), what `StreamBeam` and the CLI refuse,
and the two entry points' prototypes."""
import importlib.machinery
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('st_ctc_beam_stream_read_nbest', 'st_ctc_beam_stream_step_pieces_nbest')


def bits(x):
  return int(np.asarray([x], dtype=np.float32).view(np.int32)[0])


def record(stream, piece, old, hyps):
  """A record as the device writes it: ``hyps`` = [(whole ids, log_prob)], stored from label ``old`` on."""
  tails = [list(ids[old:]) for ids, _ in hyps]
  words = 6 + 2 * len(hyps) + sum(len(t) for t in tails)
  out = [stream, piece, len(hyps), old, words, 0]
  for ids, lp in hyps:
    out += [len(ids), bits(lp)]
  for t in tails:
    out += t
  assert len(out) == words
  return out


# stream 0 holds [7, 8] stable labels; stream 2 closes two utterances in one step (pieces 0 and 1); stream 1's list is short and
# holds the empty hypothesis
RECORDS = {
    (0, 0): (2, [([7, 8, 1, 2, 3], -1.5), ([7, 8, 1, 2], -2.25), ([7, 8], -3.0)]),
    (0, 2): (0, [([4], -0.125), ([], -0.5)]),
    (1, 2): (0, [([5, 5, 6], -7.0)]),
    (0, 1): (0, [([], 0.0)]),
}
PREFIXES = {(0, 0): [7, 8, 9], (0, 2): [], (1, 2): [], (0, 1): [], (0, 3): [1]}     # (stream 3 closed nothing: no record)


def arena_of(order, fill=-1, room=0):
  words = [w for key in order for w in record(key[1], key[0], *RECORDS[key])]
  return np.asarray(words + [fill] * room, dtype=np.int32), len(words)


def check(lists, keys):
  assert sorted(lists) == sorted(keys)
  for key in keys:
    want = RECORDS[key][1]
    assert [h['ids'] for h in lists[key]] == [list(ids) for ids, _ in want]
    assert [np.float32(h['log_prob']).tobytes() for h in lists[key]] == [np.float32(lp).tobytes() for _, lp in want]


def test_parser_reads_records_in_any_order():
  from speecht_amd import nbest
  for order in ([(0, 0), (0, 2), (1, 2), (0, 1)], [(1, 2), (0, 1), (0, 0), (0, 2)], [(0, 1), (0, 2), (0, 0), (1, 2)]):
    arena, used = arena_of(order, room=5)
    lists, lost = nbest.read_arena(arena, used, PREFIXES)
    assert lost == 0
    check(lists, order)
    assert all(isinstance(h, nbest.Hypothesis) for hyps in lists.values() for h in hyps)
    # (n below n_best: the lists are as long as their records say; the zero-length hypothesis is an empty list of ids)
    assert len(lists[(0, 2)]) == 2 and lists[(0, 2)][1]['ids'] == [] and len(lists[(0, 1)]) == 1
    # the words alone, without the room behind them, read the same
    assert nbest.read_arena(arena[:used], used, PREFIXES)[0] == lists
  assert nbest.read_arena(np.full(9, -1, np.int32), 0, PREFIXES) == ({}, 0)
  assert nbest.read_arena(np.zeros(0, np.int32), 0, {}) == ({}, 0)


def test_parser_reports_lists_beyond_the_capacity_as_lost():
  from speecht_amd import nbest
  order = [(0, 0), (0, 2), (1, 2), (0, 1)]
  full, used = arena_of(order)
  sizes = [len(record(k[1], k[0], *RECORDS[k])) for k in order]
  for fit in range(len(order)):
    # the arena ends inside record `fit`, which the device then does not write: the fill value lies there
    for cut in sorted({sum(sizes[:fit]), sum(sizes[:fit]) + 3, sum(sizes[:fit + 1]) - 1}):
      arena = np.full(cut, -1, dtype=np.int32)
      arena[:sum(sizes[:fit])] = full[:sum(sizes[:fit])]
      lists, lost = nbest.read_arena(arena, used, PREFIXES)
      check(lists, order[:fit])
      assert lost == used - sum(sizes[:fit]) > 0


def test_parser_refuses_malformed_records():
  from speecht_amd import nbest
  arena, used = arena_of([(0, 0), (0, 2)], room=4)
  first = len(record(0, 0, *RECORDS[(0, 0)]))
  def broken(at, value, used=used, prefixes=PREFIXES):
    a = arena.copy()
    if at is not None:
      a[at] = value
    with pytest.raises(nbest.ArenaError):
      nbest.read_arena(a, used, prefixes)
  broken(4, used + 1)                       # a word count that runs past `used`
  broken(first + 4, used - first + 1)       # ... by one word, in the last record
  broken(None, 0, used=used - 1)            # `used` ends inside the last record
  broken(None, 0, used=first + 3)           # ... inside a header
  broken(None, 0, used=-1)
  broken(5, 1)                              # the header's last word is 0
  broken(2, 0)                              # no hypothesis
  broken(2, 1 << 30)                        # more pairs than words
  broken(4, 6)                              # fewer words than the header and the pairs need
  broken(3, 3)                              # a hypothesis shorter than the stable labels
  broken(3, 1)                              # the tails do not fill the words
  broken(6, 9)                              # a length that does not fit its tail
  broken(0, -1)
  broken(1, -2)
  broken(0, 3, prefixes={k: v for k, v in PREFIXES.items() if k != (0, 3)})   # a final nobody expects
  broken(None, 0, prefixes={**PREFIXES, (0, 0): [7]})                 # fewer labels held than the record calls stable
  broken(first, 0)                          # a second record of the same final
  # huge counts never become indices: int32 extremes in every header field
  for at in range(6):
    for value in (np.iinfo(np.int32).max, np.iinfo(np.int32).min):
      if (at, value) != (5, 0):
        broken(at, value)


def test_stream_beam_validates_the_list_options(tmp_path):
  from speecht_amd import streaming
  S = streaming.StreamBeam
  assert S().nbest is None and S().rescore is None
  assert S(nbest=1).nbest == 1 and S(nbest=16).nbest == 16 and S(beam_width=128, nbest=128).nbest == 128
  for bad in (dict(nbest=0), dict(nbest=17), dict(nbest=-1), dict(beam_width=4, nbest=5), dict(nbest=2.0), dict(nbest=True),
              dict(nbest='3'), dict(beam_width=128, nbest=129)):
    with pytest.raises(streaming.StreamError):
      S(**bad)
  missing = str(tmp_path / 'no_such_model.arpa')                 # (a refusal comes before the model is looked for)
  for bad in (dict(rescore=dict(language_model=missing)),                                  # rescore without nbest
              dict(nbest=2, rescore={}), dict(nbest=2, rescore=dict(lm_weight=0.5)),         # ... without a model
              dict(nbest=2, rescore=dict(language_model=None)), dict(nbest=2, rescore=missing),
              dict(nbest=2, rescore=dict(language_model=missing, weight=1.0)),
              dict(nbest_words=100), dict(nbest=2, nbest_words=-1), dict(nbest=2, nbest_words=2 ** 31)):
    with pytest.raises(streaming.StreamError):
      S(**bad)
  assert S(nbest=2, nbest_words=0).nbest_words == 0
  # the second model's defaults are `transcribe`'s: the first pass's weight; its word-count weights only if it had a model
  from speecht_amd.language_model import LanguageModel
  from tests.stream_beam_cases import arpa_text
  path = tmp_path / 'second.arpa'
  path.write_text(arpa_text(3))
  lm2 = LanguageModel.load(str(path))
  r = S(nbest=2, lm_weight=0.7, rescore=dict(language_model=lm2)).rescore
  assert r['language_model'] is lm2 and (r['lm_weight'], r['word_count_weight'], r['valid_word_count_weight']) == (0.7, 0.0, 0.0)
  r = S(nbest=2, lm=lm2, lm_weight=0.7, word_count_weight=0.25, rescore=dict(language_model=str(path), lm_weight=1.5)).rescore
  assert isinstance(r['language_model'], LanguageModel)
  assert (r['lm_weight'], r['word_count_weight'], r['valid_word_count_weight']) == (1.5, 0.25, 2.3)


def test_entry_points_are_exported_with_the_bias_forms_arguments_plus_four():
  from speecht_amd import _lib
  lib = _lib.load()
  header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'speecht_hip.h')).read(), flags=re.S)
  params = lambda name: [' '.join(p.split()) for p in re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', header).group(1).split(',')]
  for name in NAMES:
    assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    base = name[:-len('nbest')] + 'bias'
    assert params(name) == params(base) + ['int n_best', 'int32_t* arena', 'int arena_words', 'int32_t* arena_used']
    restype, argtypes = _lib._SIGNATURES[name]
    assert restype is _lib._SIGNATURES[base][0]
    assert [a.__name__ for a in argtypes] == [a.__name__ for a in _lib._SIGNATURES[base][1]] + ['c_int', 'c_void_p', 'c_int', 'c_void_p']
  # the six entry points before them keep their prototypes
  for name, count in (('st_ctc_beam_stream_step', 20), ('st_ctc_beam_stream_read', 15), ('st_ctc_beam_stream_step_pieces', 24),
                      ('st_ctc_beam_stream_step_bias', 22), ('st_ctc_beam_stream_read_bias', 17), ('st_ctc_beam_stream_step_pieces_bias', 26)):
    assert len(params(name)) == count == len(_lib._SIGNATURES[name][1])
  text = ' '.join(open(os.path.join(ROOT, 'include', 'speecht_hip.h')).read().split())
  assert '{stream, piece, n, old stable_len, words of this record, 0}' in text and 'N-best lists from both beam searches' in text


def test_bad_list_arguments_return_the_error_without_a_launch():
  """Every check runs before anything is enqueued, so the refusals need no device: null pointers everywhere else are refused first
  only where an argument before them is null, and the list arguments are reached with dummy host addresses that are never read."""
  import ctypes
  from speecht_amd import _lib
  lib = _lib.load()
  buf = (ctypes.c_int64 * 64)()
  p = ctypes.cast(buf, ctypes.c_void_p)
  read = lambda n_best, arena, words, used, bias=None, roots=None, beam=16: lib.st_ctc_beam_stream_read_nbest(
      p, 1, beam, None, 0.0, 0.0, 0.0, 0.0, p, p, 10, p, 4, p, None, bias, roots, n_best, arena, words, used)
  EINVAL = lib.st_ctc_beam_stream_read_nbest(None, 1, 16, None, 0.0, 0.0, 0.0, 0.0, p, p, 10, p, 4, p, None, None, None, 1, p, 8, p)
  assert EINVAL != 0
  for args in ((0, p, 8, p), (17, p, 8, p), (-3, p, 8, p), (1, None, 8, p), (1, p, 8, None), (1, p, -1, p)):
    assert read(*args) == EINVAL, args
    assert b'n_best' in lib.st_last_error() or b'null' in lib.st_last_error() or b'arena_words' in lib.st_last_error()
  assert read(1, p, 8, p, bias=None, roots=p) == EINVAL and b'together' in lib.st_last_error()
  pieces = lambda n_best, arena, words, used: lib.st_ctc_beam_stream_step_pieces_nbest(
      p, 32, 29, p, p, 1, 0, 1, 16, 0, None, 0.0, 0.0, 0.0, 0.0, p, p, 10, None, 0, p, 4, p, None, None, None, n_best, arena, words, used)
  for args in ((0, p, 8, p), (17, p, 8, p), (1, None, 8, p), (1, p, 8, None), (1, p, -1, p)):
    assert pieces(*args) == EINVAL, args


def _cli():
  loader = importlib.machinery.SourceFileLoader('speecht_cli_stream_nbest', os.path.join(ROOT, 'speecht-cli'))
  spec = importlib.util.spec_from_loader(loader.name, loader)
  cli = importlib.util.module_from_spec(spec)
  loader.exec_module(cli)
  return cli


def test_cli_flags(capsys):
  from speecht_amd import streaming
  cli = _cli()
  _, flags = cli.parse(['stream', 'a.flac'])
  assert not hasattr(flags, 'nbest') and streaming.lists_of(flags) == {}
  _, flags = cli.parse(['stream', 'a.flac', '--beam-width', '8', '--nbest', '3'])
  assert streaming.lists_of(flags) == dict(nbest=3)
  _, flags = cli.parse(['stream', 'a.flac', '--language-model', 'lm.arpa', '--nbest', '100', '--rescore-language-model', 'big.arpa'])
  assert streaming.lists_of(flags) == dict(nbest=100, rescore=dict(language_model='big.arpa', lm_weight=flags.lm_weight,
                                                                   word_count_weight=flags.word_count_weight,
                                                                   valid_word_count_weight=flags.valid_word_count_weight))
  _, flags = cli.parse(['stream', 'a.flac', '--hotword', 'anna', '--nbest', '16', '--rescore-language-model', 'big.arpa',
                        '--rescore-lm-weight', '1.25'])
  assert streaming.lists_of(flags)['rescore']['lm_weight'] == 1.25
  # refused with a message and status 1, before any model is built: --nbest without a search, outside the beam, the companions alone
  for args in (['--nbest', '3'], ['--beam-width', '8', '--nbest', '9'], ['--beam-width', '8', '--nbest', '0'],
               ['--language-model', 'lm.arpa', '--nbest', '101'], ['--hotword', 'anna', '--nbest', '17'],
               ['--beam-width', '8', '--rescore-language-model', 'big.arpa'], ['--beam-width', '8', '--rescore-lm-weight', '1.0'],
               ['--beam-width', '8', '--nbest', '2', '--rescore-lm-weight', '1.0']):
    capsys.readouterr()
    assert cli.main(['stream', 'a.flac'] + args) == 1, args
    out = capsys.readouterr()
    assert out.out == '' and out.err.startswith('stream: --'), (args, out)
  assert streaming.nbest_lines('a.flac', None) == []
  from speecht_amd import nbest
  lines = streaming.nbest_lines('a.flac', [nbest.Hypothesis(ids=[0, 1], log_prob=-1.25), nbest.Hypothesis(ids=[], log_prob=-3.0)])
  assert lines == ['a.flac\t1\t-1.2500\tab', 'a.flac\t2\t-3.0000\t']


def test_components_takes_a_phrase_set_per_list():
  """`nbest.components` with one `Hotwords` (or None) per list gives each list what the single-set form gives it."""
  from speecht_amd import nbest
  from speecht_amd.hotwords import Hotwords
  hot = Hotwords(['ab'], weight=2.0)
  lists = [[([0, 1], -1.0), ([0], -2.0)], [([0, 1, 2], -0.5)]]
  both = nbest.components(None, None, lists, hotwords=[hot, None])
  assert both[0] == nbest.components(None, None, lists[:1], hotwords=hot)[0]
  assert both[1] == nbest.components(None, None, lists[1:])[0] and 'bias' not in both[1][0]
  with pytest.raises(ValueError):
    nbest.components(None, None, lists, hotwords=[hot])


def test_a_failed_finals_record_beside_a_good_one_costs_nothing():
  """The device writes a finishing read-out's record whatever its status and however long its tail; the host gives up on such a final
  and names its key as unwanted.  The record is stepped over: the good list comes out, nothing is raised, nothing counts as lost."""
  from speecht_amd import nbest, streaming
  long_tail = [([1] * 300, -4.0), ([2] * 299, -5.0)]               # (more labels than any max_tail: well formed all the same)
  for order in ([(0, 1), (0, 0)], [(0, 0), (0, 1)]):
    words = []
    for key in order:
      words += record(0, 0, *RECORDS[(0, 0)]) if key == (0, 0) else record(1, 0, 0, long_tail)
    arena = np.asarray(words + [-1] * 3, dtype=np.int32)
    with pytest.raises(nbest.ArenaError):
      nbest.read_arena(arena, len(words), {(0, 0): [7, 8]})          # unannounced, the record is none the caller expects
    lists, lost = nbest.read_arena(arena, len(words), {(0, 0): [7, 8]}, skip={(0, 1), (3, 1)})
    assert lost == 0
    check(lists, [(0, 0)])
    # the failed record first and the arena too small for the second: the parser still walks past it
    cut = len(record(1, 0, 0, long_tail)) + 2
    if order[0] == (0, 1):
      lists, lost = nbest.read_arena(arena[:cut], len(words), {(0, 0): [7, 8]}, skip={(0, 1)})
      assert lists == {} and lost == len(words) - (cut - 2)
    # a skipped record must be well formed too, and may come once
    bad = arena.copy()
    bad[words.index(300) if 300 in words else 0] = 7 if 300 in words else -1
    with pytest.raises(nbest.ArenaError):
      nbest.read_arena(bad, len(words), {(0, 0): [7, 8]}, skip={(0, 1)})
    twice = np.asarray(words + record(1, 0, 0, long_tail), dtype=np.int32)
    with pytest.raises(nbest.ArenaError):
      nbest.read_arena(twice, len(twice), {(0, 0): [7, 8]}, skip={(0, 1)})
    # the recogniser's own step from arena to results, on a recogniser that owns no device: the good final gets its list
    rec = object.__new__(streaming._BeamPart)
    rec.beam, rec.engine, rec.slot_set = streaming.StreamBeam(beam_width=4, nbest=3), None, np.zeros(2, np.int64)
    result = streaming.StepResult()
    result.nbest, result.nbest_lost = {0: None, 1: None}, {0: 0, 1: 0}
    rec.hyp, rec.logp, rec.stable = [[], []], np.zeros(2, np.float32), np.zeros(2, np.int64)
    rec.final_lists(arena[:len(words)], len(words), [(0, (0, 0), [7, 8], None)], result, {(0, 1)})
    assert [h['ids'] for h in result.nbest[0]] == [list(i) for i, _ in RECORDS[(0, 0)][1]] and result.nbest[1] is None
    assert result.nbest_lost == {0: 0, 1: 0} and all(h['acoustic'] == h['log_prob'] for h in result.nbest[0])
