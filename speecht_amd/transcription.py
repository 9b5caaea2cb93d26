"""Audio files to text: `speecht-cli transcribe` and its Python API.

Decoding the container stays on the host (audio_io: FLAC / 16-bit wav / npy, at the file's own rate).  Everything after it
runs on the device: librosa.load's resampling to the model's rate (the kaiser_best kernel, audio_io.resample_kaiser_best_device),
the features (power spectrogram or MFCCs, preprocessing.power_spectrogram_device / mfccs_device), the network and the decoder
(inference.transcribe) -- the audio goes to the device once and only the features come back.

Batch semantics: nothing in the network is masked, so the logits near an utterance's end depend on the padded length of the
batch it is in.  The default ``batch_size=1`` runs every file as one [1, T, C] batch without padding -- what the reference's
`record` does with its single utterance.  ``batch_size > 1`` buckets files by length for throughput; transcripts near the ends
of the shorter files of a bucket may then differ from the ``batch_size=1`` ones -- unless ``mask_padding`` (``--mask-padding``)
is set: the forward pass then zeroes every utterance's rows past its own length after every layer, and a batched utterance gets
the logits it would get alone.

Long recordings: ``segment`` (``--segment``) cuts every file into utterances at its silences on the device
(segmentation.segment_device: the endpointing rules of the reference's `record`), transcribes the utterances like files and
joins their texts; ``--segment --batch-size N --mask-padding`` is the combination for them.
"""
import contextlib
import json
import os
import sys
import time

from . import audio_io, inference, preprocessing, segmentation

AUDIO_EXTENSIONS = ('.flac', '.wav')          # what a directory is searched for
FEATURE_WIDTH = {'power': 128, 'mfcc': 39}
N_FFT = 512
FEATURE_BATCH = 64                            # utterances per resample + feature launch sequence


class TranscriptionError(ValueError):
  """A file that cannot be transcribed: unreadable, or too short for the features."""


def expand_paths(paths):
  """PATH arguments -> audio files in order: a file stays as given, a directory becomes its *.flac and *.wav files, searched
  recursively, in sorted order."""
  files = []
  for p in paths:
    if os.path.isdir(p):
      found = []
      for root, _, names in os.walk(p):
        found += [os.path.join(root, n) for n in names if os.path.splitext(n)[1].lower() in AUDIO_EXTENSIONS]
      files += sorted(found)
    else:
      files.append(p)
  return files


def load_native(path):
  """(float32 mono samples, native rate): preprocessing.load_audio without the host resampler."""
  if not os.path.isfile(path):
    raise TranscriptionError('{}: no such file'.format(path))
  ext = os.path.splitext(path)[1].lower()
  try:
    if ext == '.flac':
      return audio_io.librosa_load(path, sr=None)
    if ext in ('.wav', '.npy'):
      return preprocessing.load_audio(path)
  except Exception as e:                      # a corrupt file is reported with its path; the other files go on
    raise TranscriptionError('{}: cannot decode: {}'.format(path, e)) from e
  raise TranscriptionError('{}: unsupported audio file type {} (expected .flac, 16-bit .wav or .npy)'.format(
      path, ext or '(none)'))


def _target_rate(rate, sample_rate):
  return rate if sample_rate in (None, 'native') else int(sample_rate)


def check_length(n, rate, sample_rate, name='utterance'):
  """Raise TranscriptionError if n samples at ``rate`` are too short for the features after resampling (<= n_fft / 2)."""
  target = _target_rate(rate, sample_rate)
  length = audio_io.resample_lengths(int(n), int(rate), target)[1]
  if length <= N_FFT // 2:
    raise TranscriptionError('{}: too short: {} samples at {} Hz (the features need more than {})'.format(
        name, length, target, N_FFT // 2))


def device_features(signals, rates, feature_type='power', sample_rate=22050, device='cuda:0'):
  """Features of float32 mono signals at their own rates: resampled to ``sample_rate`` (None / 'native': kept at their own
  rate) and turned into [T, 128] power spectrograms or [T, 39] MFCCs on the device, FEATURE_BATCH signals per launch
  sequence (signals of one target rate share a launch).  Returns a list of host arrays in input order."""
  if feature_type not in FEATURE_WIDTH:
    raise ValueError('feature_type must be power or mfcc, got {!r}'.format(feature_type))
  extract = preprocessing.power_spectrogram_device if feature_type == 'power' else preprocessing.mfccs_device
  for i, (s, r) in enumerate(zip(signals, rates)):
    check_length(len(s), r, sample_rate, 'utterance {}'.format(i))
  targets = [_target_rate(r, sample_rate) for r in rates]
  feats = [None] * len(signals)
  for target in sorted(set(targets)):
    idx = [i for i, t in enumerate(targets) if t == target]
    for k in range(0, len(idx), FEATURE_BATCH):
      part = idx[k:k + FEATURE_BATCH]
      audio, offsets = audio_io.resample_kaiser_best_device([signals[i] for i in part], [rates[i] for i in part], target, device)
      for i, f in zip(part, extract(audio, offsets, target)):
        feats[i] = f
  return feats


def device_features_on_device(audio, offsets, rates, feature_type='power', sample_rate=22050):
  """device_features for signals that are already on the device (the layout segmentation.segment_device returns: ``audio`` a float32
  device tensor, signal i at [offsets[i], offsets[i + 1]) at rates[i]): no trip through the host between the gather, the resampler
  and the features.  A signal too short for the features gets None."""
  if feature_type not in FEATURE_WIDTH:
    raise ValueError('feature_type must be power or mfcc, got {!r}'.format(feature_type))
  extract = preprocessing.power_spectrogram_device if feature_type == 'power' else preprocessing.mfccs_device
  n = len(rates)
  feats = [None] * n
  targets = [_target_rate(int(r), sample_rate) for r in rates]

  def long_enough(i):
    return audio_io.resample_lengths(int(offsets[i + 1] - offsets[i]), int(rates[i]), targets[i])[1] > N_FFT // 2

  i = 0
  while i < n:
    # consecutive signals of one target rate share a launch sequence, FEATURE_BATCH at the most (their samples are one range)
    j = i
    while j < n and j - i < FEATURE_BATCH and targets[j] == targets[i] and long_enough(j):
      j += 1
    if j == i:                                  # too short: left out
      i += 1
      continue
    resampled, out_offsets = audio_io.resample_device(audio, offsets[i:j + 1], rates[i:j], targets[i])
    for k, f in enumerate(extract(resampled, out_offsets, targets[i])):
      feats[i + k] = f
    i = j
  return feats


def _segmented(engine, signals, rates, options, feature_type, sample_rate, batch_size, timestamps, mask_padding, decode,
               confidence=False):
  """Segment every signal at its own rate, transcribe the utterances like files -> per signal a list of dicts {start, end (seconds
  in the signal), text, ids} in time order; with ``timestamps`` also ``words`` ([{word, start, end}] in seconds of the signal; None
  where the text is too long to align).  An utterance too short for the features has an empty text.  ``confidence``: also
  ``confidence`` ({'log_prob', 'words'} of inference.transcribe, None where the text is too long or empty) and, in ``words``, each
  word's `confidence` (without ``timestamps``: ``words`` = [{word, confidence}])."""
  table, gathered, out_offsets = segmentation.segment_audio(signals, rates, options, engine.device)
  out = [[] for _ in signals]
  if len(table) == 0:
    return out
  seg_rates = [int(rates[i]) for i in table[:, 0]]
  feats = device_features_on_device(gathered, out_offsets, seg_rates, feature_type, sample_rate)
  ok = [s for s, f in enumerate(feats) if f is not None]
  res = inference.transcribe(engine, [feats[s] for s in ok], batch_size=batch_size, timestamps=timestamps, mask_padding=mask_padding,
                             **dict(decode, **(dict(confidence=True) if confidence else {}))) if ok else ([], [], [], [])
  found = {s: k for k, s in enumerate(ok)}
  for s, (i, a, b) in enumerate(table.tolist()):
    rate = float(rates[i])
    seg = dict(start=a / rate, end=b / rate, text='', ids=[])
    if timestamps or confidence:
      seg['words'] = []
    if confidence:
      seg['confidence'] = None
    if s in found:
      k = found[s]
      seg['ids'], seg['text'] = res[0][k], res[1][k]
      conf = res[-1][k] if confidence else None
      if confidence:
        from . import alignment
        seg['confidence'] = conf
        if not timestamps:
          seg['words'] = alignment.confident_words(seg['ids'], conf['words']) if conf is not None else None
      if timestamps:
        from . import alignment
        spans, target = res[2][k], _target_rate(int(rates[i]), sample_rate)
        seg['spans'], seg['frames'] = spans, feats[s].shape[0] // 2
        if spans is None:
          seg['words'] = None
        else:
          inside = alignment.timed_words(seg['ids'], spans, target, (out_offsets[s + 1] - out_offsets[s]) / rate,
                                         confidence=conf['words'] if conf is not None else None)
          seg['words'] = segmentation.stitch(inside, seg['start'], segmentation.pad_samples(options, rates[i]) / rate, len(signals[i]) / rate)
    out[i].append(seg)
  return out


def _join_segments(segments):
  """(ids, text) of a segmented signal: the non-empty segment texts joined by one space."""
  from . import vocabulary
  ids = []
  for seg in segments:
    if seg['text']:
      ids += ([vocabulary.SPACE_ID] if ids else []) + list(seg['ids'])
  return ids, ' '.join(seg['text'] for seg in segments if seg['text'])


def transcribe_audio(engine, signals, rates, feature_type='power', sample_rate=22050, batch_size=1, mask_padding=False, segment=None,
                     **decode):
  """Transcribe float32 mono signals in [-1, 1] at the given source rates -> (list of id lists, list of strings).

  Resampling (to ``sample_rate``, default 22 050 Hz as librosa.load; None or 'native' keeps each signal's rate) and the
  features run on the engine's device; the features must match the engine's input width (power: 128, mfcc: 39).
  ``decode``: inference.transcribe's decoding arguments -- none (greedy), ``beam_width``, or ``language_model`` with
  ``lm_options``; and ``hotwords``, which biases the beam search towards given phrases.

  ``batch_size=1`` (default): every signal is one [1, T, C] batch without padding, the semantics of the reference's `record`.
  ``batch_size > 1``: signals are bucketed by length into padded batches for throughput; nothing in the network is masked,
  so transcripts near the ends of the shorter signals of a batch may differ from the ``batch_size=1`` ones -- unless
  ``mask_padding`` is set (inference.transcribe).

  ``segment``: a segmentation.SegmentOptions -- every signal is cut into utterances at its silences on the device, the utterances
  are transcribed like signals, and a signal's ids / text are those of its utterances joined by one space."""
  if segment is not None:
    joined = [_join_segments(segs) for segs in _segmented(engine, signals, rates, segment, feature_type, sample_rate, batch_size,
                                                          False, mask_padding, decode)]
    return [j[0] for j in joined], [j[1] for j in joined]
  feats = device_features(signals, rates, feature_type, sample_rate, engine.device)
  return inference.transcribe(engine, feats, batch_size=batch_size, mask_padding=mask_padding, **decode)


def transcribe_files(engine, paths, feature_type='power', sample_rate=22050, batch_size=1, timings=None, timestamps=False,
                     mask_padding=False, segment=None, confidence=False, nbest=None, rescore=None, **decode):
  """Transcribe audio files (.flac, 16-bit .wav, .npy taken as 16 kHz) -> a list, in ``paths`` order, of dicts
  {path, seconds, text, ids, error}: ``error`` is the message for a file that cannot be read or is too short (its text and
  ids are None); the other files are transcribed as transcribe_audio does (same arguments, same batch semantics).
  ``timestamps=True`` adds ``spans`` ([L, 2] output frames per id, inference.transcribe; None when the text is too long to align),
  ``frames`` and ``sample_rate`` (the rate of the features), which `alignment.timed_words` turns into word times.
  ``timings``: a dict that receives the seconds spent in host decoding ('decode_host'), resampling and features
  ('features') and the network with the decoder ('transcribe').
  ``mask_padding``: as transcribe_audio.  ``segment`` (a segmentation.SegmentOptions): every file is segmented at its own rate,
  before resampling, and its entry gains ``segments``: [{start, end, text, ids}] in seconds of the file and time order (with
  ``timestamps`` also ``words``, the word times in the file: segment start minus pad plus the time inside the segment, clipped to
  the file; segments are short, so files of any length can be aligned).  ``text`` / ``ids`` are the non-empty segment texts joined
  by one space; a file without a segment has an empty text and is no error; ``spans`` is None (the words are per segment).
  Segmentation is timed with 'features', the rest with 'transcribe'.
  ``confidence=True`` adds ``confidence``: {'log_prob', 'words': [probability per word of the text]} (inference.transcribe; None
  when the text is too long), which `alignment.timed_words` / `alignment.confident_words` put next to each word; under ``segment``
  it is per segment and the words of ``segments`` carry `confidence`.
  ``nbest=N`` (with a beam search; not with ``segment``: per-segment lists do not join into file lists) adds ``nbest``: the file's up
  to N best hypotheses, best first (inference.transcribe: dicts with 'text', 'log_prob', 'acoustic' and the LM parts); ``rescore``
  re-ranks them under a second model first, and ``text`` / ``ids`` are the best hypothesis after that.
  ``hotwords`` (among ``decode``; a `hotwords.Hotwords` or a list of phrases): the beam search is biased towards the phrases
  (inference.transcribe); it composes with ``segment``, ``timestamps``, ``confidence`` and ``nbest``, whose hypotheses then carry 'bias'."""
  if nbest is not None and segment is not None:
    raise ValueError('transcribe_files: nbest is not available with segment (per-segment lists do not join into file lists)')
  results = []
  signals, rates, ok = [], [], []
  t0 = time.perf_counter()
  for path in paths:
    entry = dict(path=path, seconds=None, text=None, ids=None, error=None)
    results.append(entry)
    try:
      samples, rate = load_native(path)
      entry['seconds'] = len(samples) / float(rate)
      check_length(len(samples), rate, sample_rate, path)
    except TranscriptionError as e:
      entry['error'] = str(e)
      continue
    signals.append(samples)
    rates.append(rate)
    ok.append(entry)
  t1 = time.perf_counter()
  if ok and segment is not None:
    t2 = t1
    per_file = _segmented(engine, signals, rates, segment, feature_type, sample_rate, batch_size, timestamps, mask_padding, decode,
                          confidence)
    for entry, rate, segs in zip(ok, rates, per_file):
      entry['segments'] = segs
      entry['ids'], entry['text'] = _join_segments(segs)
      if timestamps:
        entry.update(spans=None, frames=None, sample_rate=_target_rate(rate, sample_rate))
      if confidence:
        entry['confidence'] = None
  elif ok:
    feats = device_features(signals, rates, feature_type, sample_rate, engine.device)
    t2 = time.perf_counter()
    lists = dict(nbest=nbest, rescore=rescore) if nbest is not None else {}
    res = inference.transcribe(engine, feats, batch_size=batch_size, timestamps=timestamps, mask_padding=mask_padding,
                               **dict(decode, **dict(lists, **(dict(confidence=True) if confidence else {}))))
    if nbest is not None:
      for entry, hyps in zip(ok, res[-1]):
        entry['nbest'] = hyps
      res = res[:-1]
    for entry, i, t in zip(ok, res[0], res[1]):
      entry['ids'], entry['text'] = i, t
    if timestamps:
      for entry, f, rate, sp in zip(ok, feats, rates, res[2]):
        entry.update(spans=sp, frames=f.shape[0] // 2, sample_rate=_target_rate(rate, sample_rate))
    if confidence:
      for entry, rate, c in zip(ok, rates, res[-1]):
        entry.update(confidence=c, sample_rate=_target_rate(rate, sample_rate))
  else:
    t2 = t1
  if timings is not None:
    timings.update(decode_host=t1 - t0, features=t2 - t1, transcribe=time.perf_counter() - t2)
  return results


def run_cli(flags):
  """`speecht-cli transcribe`: prints path<TAB>transcript per file in input order (and JSON lines to --output); a file that
  cannot be transcribed is reported on stderr and makes the exit status 1.  Creates no train / data / log directory."""
  from .speech_input import SingleInputLoader
  from .speech_model import Session, create_default_model
  paths = expand_paths(flags.paths)
  if not paths:
    print('transcribe: no audio files found in {}'.format(' '.join(flags.paths)), file=sys.stderr)
    return 1
  input_size = FEATURE_WIDTH[flags.feature_type]
  with contextlib.redirect_stdout(sys.stderr):          # stdout carries the transcripts only
    model = create_default_model(flags, input_size, SingleInputLoader(input_size))
  decode = {}
  if model.language_model is not None:
    decode = dict(language_model=model.language_model, beam_width=model.beam_width,
                  lm_options=dict(input_transform=model.beam_input, lm_weight=model.lm_weight,
                                  word_count_weight=model.word_count_weight,
                                  valid_word_count_weight=model.valid_word_count_weight))
  elif model.beam_width:
    decode = dict(beam_width=model.beam_width)
  from . import hotwords
  bias = hotwords.from_flags(flags)
  if bias is not None:
    decode['hotwords'] = bias                           # (inference.transcribe: beam 16 when no beam search was asked for)
  with Session(flags.device) as sess:
    with contextlib.redirect_stdout(sys.stderr):
      model.restore(sess, flags.run_train_dir)          # FileNotFoundError('No checkpoint for evaluation found'), as evaluate
    timestamps = bool(getattr(flags, 'timestamps', False))
    confidence = bool(getattr(flags, 'confidence', False))
    segment = None
    if getattr(flags, 'segment', False):
      segment = segmentation.SegmentOptions(threshold=flags.segment_threshold, min_silence=flags.min_silence,
                                            max_segment=flags.max_segment)
    nbest = getattr(flags, 'nbest', None)
    rescore = None
    if nbest and getattr(flags, 'rescore_language_model', None):
      shared = model.language_model is not None
      rescore = dict(language_model=flags.rescore_language_model,
                     lm_weight=getattr(flags, 'rescore_lm_weight', model.lm_weight),
                     word_count_weight=model.word_count_weight if shared else flags.word_count_weight,
                     valid_word_count_weight=model.valid_word_count_weight if shared else flags.valid_word_count_weight)
    results = transcribe_files(model.engine, paths, flags.feature_type, flags.sample_rate, flags.batch_size, timestamps=timestamps,
                               mask_padding=bool(getattr(flags, 'mask_padding', False)), segment=segment, confidence=confidence,
                               **dict(decode, **(dict(nbest=nbest, rescore=rescore) if nbest else {})))
  out = open(flags.output, 'w') if flags.output else None
  status = 0
  try:
    for r in results:
      if r['error'] is not None:
        print('transcribe: {}'.format(r['error']), file=sys.stderr)
        status = 1
        continue
      print('{}\t{}'.format(r['path'], r['text']), flush=True)
      line = dict(path=r['path'], seconds=r['seconds'], text=r['text'])
      if r.get('nbest') is not None:
        parts = ('text', 'log_prob', 'acoustic', 'lm_log10', 'words', 'valid_words', 'bias')
        line['nbest'] = [{k: h[k] for k in parts if k in h} for h in r['nbest']]
        for rank, h in enumerate(r['nbest'], 1):
          print('{}\t{}\t{:.4f}\t{}'.format(r['path'], rank, h['log_prob'], h['text']), flush=True)
      if confidence and r.get('confidence') is not None:
        line['log_prob'] = r['confidence']['log_prob']
      if segment is not None:
        line['segments'] = []
        for seg in r['segments']:
          item = dict(start=round(seg['start'], 4), end=round(seg['end'], 4), text=seg['text'])
          if confidence and seg.get('confidence') is not None:
            item['log_prob'] = seg['confidence']['log_prob']
          if (timestamps or confidence) and seg['words'] is not None:
            item['words'] = seg['words']
            for w in seg['words']:
              times = '{:.3f}\t{:.3f}'.format(w['start'], w['end']) if 'start' in w else '-\t-'
              tail = '\t{:.4f}'.format(w['confidence']) if 'confidence' in w else ''
              print('{}\t{}\t{}{}'.format(r['path'], times, w['word'], tail), flush=True)
          line['segments'].append(item)
      elif (timestamps and r['spans'] is not None) or (confidence and r.get('confidence') is not None):
        from . import alignment
        alignment.print_words(r)
        line['words'] = alignment.result_json(r)['words']
      if out:
        out.write(json.dumps(line) + '\n')
  finally:
    if out:
      out.close()
  return status
