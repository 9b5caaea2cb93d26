"""Silence segmentation on the GPU (csrc/segment.hip) against its numpy specification (tests/segment_oracle.py): the segment
table must be identical and the gathered utterances bit-identical; then `transcribe_files(segment=...)` end to end.

Shapes are tiny: rate 1000 makes a chunk 20 samples; min_silence 0.1 s is G = 5 chunks and max_segment 0.2 s is M = 10 chunks."""
import os
import wave

import numpy as np
import pytest
import torch

from tests import segment_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_FLAC = os.path.join(ROOT, 'tests', 'golden', '1089-134686-0037.flac')
SMALL = dict(threshold=0.03, min_silence=0.1, max_segment=0.2)
G, M = 5, 10


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def build(rng, pattern, chunk=20, tail=0):
  """pattern: (kind, chunks) pairs -- 'loud': samples of 0.3..1 in magnitude, 'quiet': of at most 0.01, 'flat': every sample 0.5
  (equal chunk peaks: ties); ``tail``: further loud samples, a last partial chunk."""
  parts = []
  for kind, count in pattern:
    n = count * chunk
    if kind == 'loud':
      parts.append(rng.uniform(0.3, 1.0, n) * rng.choice([-1.0, 1.0], n))
    elif kind == 'flat':
      parts.append(np.full(n, 0.5))
    else:
      parts.append(rng.uniform(-0.01, 0.01, n))
  if tail:
    parts.append(rng.uniform(0.3, 1.0, tail))
  return np.concatenate(parts + [np.zeros(0)]).astype(np.float32)


def check(dev, signals, rates, pad=0.1, **options):
  """The device against the specification: -> the table."""
  from speecht_amd.segmentation import SegmentOptions, segment_audio
  opts = SegmentOptions(pad=pad, **options)
  table, gathered, out_offsets = segment_audio(signals, rates, opts, dev)
  want, counts = O.segment(signals, rates, opts.threshold, opts.min_silence, opts.max_segment)
  assert table.dtype == np.int64 and table.tolist() == want.tolist()
  utts, _ = O.gather(signals, rates, want, pad)
  lens = [len(u) for u in utts]
  assert out_offsets.tolist() == np.concatenate([[0], np.cumsum(lens)]).astype(np.int64).tolist()
  got = gathered.cpu().numpy()
  assert got.dtype == np.float32 and got.shape == (sum(lens),)
  flat = np.concatenate(utts + [np.zeros(0, np.float32)])
  assert np.array_equal(got.view(np.uint32), flat.view(np.uint32))
  return table


def test_lengths_around_a_chunk(dev):
  rng = np.random.default_rng(3)
  lengths = [0, 1, 7, 19, 20, 21, 60, 61, 64 * 20, 64 * 20 + 1, 65 * 20]
  signals = [build(rng, [('loud', 0)], tail=n) for n in lengths]
  table = check(dev, signals, [1000] * len(lengths), **SMALL)
  assert set(table[:, 0].tolist()) == set(range(1, len(lengths)))            # every signal but the empty one has segments
  # the only active sample is the very last one: of a whole number of chunks, of a partial chunk, of chunk 64
  for n in (1, 20, 40, 41, 64 * 20, 64 * 20 + 1):
    x = np.zeros(n, np.float32)
    x[-1] = -0.7
    assert check(dev, [x], [1000], **SMALL).tolist() == [[0, n - 1, n]]


def test_gaps_and_runs_across_mask_words(dev):
  rng = np.random.default_rng(5)
  signals = [
      build(rng, [('loud', 1), ('quiet', G - 1), ('loud', 1)]),                               # joins
      build(rng, [('loud', 1), ('quiet', G), ('loud', 1)]),                                   # splits
      build(rng, [('quiet', 60), ('loud', 8), ('quiet', 3), ('loud', 2)]),                    # a run across chunks 63 / 64
      build(rng, [('quiet', 61), ('loud', 2), ('quiet', G - 1), ('loud', 1)]),                # a gap of G - 1 across 63 / 64
      build(rng, [('quiet', 61), ('loud', 2), ('quiet', G), ('loud', 1)]),                    # a gap of G across 63 / 64
      build(rng, [('loud', 1), ('quiet', 62), ('loud', 1), ('quiet', 0), ('loud', 1)]),       # starts at 63 and 64 side by side
      build(rng, [('quiet', 124), ('loud', 7), ('quiet', G), ('loud', 3)]),                   # a run across 127 / 128
      build(rng, [('quiet', 125), ('loud', 1), ('quiet', G - 1), ('loud', 1), ('quiet', G), ('loud', 1)]),   # gaps across 127 / 128
      build(rng, [('loud', 1), ('quiet', 200), ('loud', 1)]),                                 # whole silent words between
      np.zeros(64 * 20, np.float32),                                                          # nothing active
  ]
  table = check(dev, signals, [1000] * len(signals), **SMALL)
  per = [table[table[:, 0] == i, 1:].tolist() for i in range(len(signals))]
  assert len(per[0]) == 1 and len(per[1]) == 2 and len(per[3]) == 1 and len(per[4]) == 2 and len(per[9]) == 0


def test_cuts(dev):
  rng = np.random.default_rng(7)
  signals = [
      build(rng, [('loud', M)]),                                                    # kept whole
      build(rng, [('loud', M + 1)]),                                                # cut once
      build(rng, [('loud', 3 * M)]),                                                # cut again and again
      build(rng, [('flat', M + 1)]),                                                # every chunk of the window ties: the earliest
      build(rng, [('flat', 3 * M + 7)]),
      build(rng, [('quiet', 58), ('flat', 2 * M + 3)]),                             # windows across chunks 63 / 64
      build(rng, [('loud', 6), ('quiet', 2), ('loud', 6)]),                         # the quietest chunk is a silent one
      build(rng, [('quiet', 120), ('loud', 4), ('quiet', G - 1), ('loud', 4), ('quiet', G - 1), ('loud', 9)]),   # cut in a run with gaps
  ]
  table = check(dev, signals, [1000] * len(signals), **SMALL)
  per = [table[table[:, 0] == i, 1:].tolist() for i in range(len(signals))]
  assert per[0] == [[0, M * 20]] and per[3] == [[0, 100], [100, 220]] and len(per[1]) == 2 and len(per[2]) >= 3
  # ... and with the default 15 / 1000 chunks on the same signals: nothing is long enough to cut
  check(dev, signals, [1000] * len(signals))


def test_silent_signal_between_active_ones_and_mixed_rates(dev):
  rng = np.random.default_rng(9)
  a = build(rng, [('loud', 3), ('quiet', 9), ('loud', 2)])
  table = check(dev, [a, np.zeros(500, np.float32), np.zeros(0, np.float32), a[::-1].copy()], [1000] * 4, **SMALL)
  assert sorted(set(table[:, 0].tolist())) == [0, 3]
  # rates 1000, 8000 and 16000 in one call: chunks of 20, 160 and 320 samples; odd lengths, odd offsets
  signals = [
      build(rng, [('loud', 2), ('quiet', 6), ('loud', 3)], 20, tail=3),
      build(rng, [('quiet', 1), ('loud', 12), ('quiet', 5), ('loud', 1)], 160, tail=77),
      build(rng, [('loud', 1), ('quiet', 4), ('loud', 11), ('quiet', 2)], 320, tail=1),
      build(rng, [('loud', 1)], 20, tail=0)[:13],
  ]
  check(dev, signals, [1000, 8000, 16000, 1000], **SMALL)
  check(dev, signals, [1000, 8000, 16000, 1000], pad=0.0, **SMALL)
  check(dev, signals, [1000, 8000, 16000, 1000])                               # the defaults


def test_signal_of_more_than_64_words(dev):
  rng = np.random.default_rng(13)
  pattern = []
  while sum(n for _, n in pattern) <= 64 * 64 + 100:
    pattern += [('loud', int(rng.integers(1, 25))), ('quiet', int(rng.integers(1, 12)))]
  x = build(rng, pattern, tail=5)
  assert -(-len(x) // 20) > 64 * 64
  table = check(dev, [x, x[:777]], [1000, 1000], **SMALL)
  assert len(table) > 100


# ---- end to end ------------------------------------------------------------------------------------------------------------------

def _wav(path, samples, rate):
  with wave.open(str(path), 'wb') as w:
    w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
    w.writeframes((np.clip(samples, -1, 1) * 32767).astype('<i2').tobytes())


def _model(tmp_path, input_size=128, seed=1234):
  from speecht_amd.speech_input import SingleInputLoader
  from speecht_amd.speech_model import Wav2LetterModel
  loader = SingleInputLoader(input_size)
  model = Wav2LetterModel(loader, input_size, 29)
  model.add_training_ops()
  model.add_decoding_ops()
  model.finalize(str(tmp_path / 'log'), 'r', 'record')
  model.init_seed = seed
  return model


def test_transcribe_files_segmented(dev, tmp_path):
  """A wav of three tone bursts with 0.5 s gaps and the golden FLAC: per segment the ids transcribe_audio gives for that segment's
  gathered audio alone, word times in file order."""
  from speecht_amd.segmentation import SegmentOptions, segment_audio
  from speecht_amd.speech_model import Session
  from speecht_amd.transcription import load_native, transcribe_audio, transcribe_files
  rate = 16000
  t = np.arange(int(0.8 * rate)) / float(rate)
  burst = lambda f0: 0.6 * np.sin(2 * np.pi * f0 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3.0 * t))
  gap = np.zeros(rate // 2)
  bursts = np.concatenate([gap, burst(300.0), gap, burst(700.0), gap, burst(1100.0), gap])
  path = tmp_path / 'bursts.wav'
  _wav(path, bursts, rate)
  paths = [str(path), GOLDEN_FLAC]
  opts = SegmentOptions()
  model = _model(tmp_path)
  with Session(dev) as sess:
    model.init_session(sess)
    eng = model.engine
    results = transcribe_files(eng, paths, batch_size=4, mask_padding=True, timestamps=True, segment=opts)
    plain = transcribe_files(eng, paths, batch_size=4, mask_padding=True, segment=opts)
    assert [r['error'] for r in results] == [None, None]
    assert len(results[0]['segments']) == 3
    for r, p in zip(results, plain):
      signal, native = load_native(r['path'])
      table, gathered, out_offsets = segment_audio([signal], [native], opts, dev)
      want_table, _ = O.segment([signal], [native])
      assert table.tolist() == want_table.tolist() and len(table) == len(r['segments']) >= 1
      host = gathered.cpu().numpy()
      alone = [host[out_offsets[s]:out_offsets[s + 1]] for s in range(len(table))]
      ids, texts = transcribe_audio(eng, alone, [native] * len(alone), batch_size=1)
      assert [seg['ids'] for seg in r['segments']] == ids
      assert [seg['ids'] for seg in p['segments']] == ids and 'words' not in p['segments'][0]
      assert r['text'] == ' '.join(x for x in texts if x) == p['text']
      for seg, (_, a, b) in zip(r['segments'], table.tolist()):
        assert seg['start'] == a / float(native) and seg['end'] == b / float(native)
      times = [w[k] for seg in r['segments'] for w in (seg['words'] or []) for k in ('start', 'end')]
      assert all(0.0 <= x <= r['seconds'] for x in times)
      starts = [w['start'] for seg in r['segments'] for w in (seg['words'] or [])]
      assert starts == sorted(starts)
    # the bursts sit where they were put (to a chunk of 20 ms and the trim)
    for seg, k in zip(results[0]['segments'], range(3)):
      assert abs(seg['start'] - (0.5 + 1.3 * k)) < 0.03 and abs(seg['end'] - (1.3 + 1.3 * k)) < 0.03
    # a file of silence has no segment, an empty text and no error
    silent = tmp_path / 'silent.wav'
    _wav(silent, np.zeros(rate), rate)
    r, = transcribe_files(eng, [str(silent)], segment=opts)
    assert r['error'] is None and r['text'] == '' and r['segments'] == [] and r['ids'] == []
