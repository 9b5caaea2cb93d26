"""Forced alignment: when each word of a known transcript was said -- `speecht-cli align` and its Python API -- and the word
times of `speecht-cli transcribe --timestamps`.

The alignment itself is the best CTC path of the transcript's ids against the network's logits (`engine.align`,
st_ctc_align_f32; semantics and tie rules: include/speecht_hip.h).  This module turns its per-character frame spans into words
and seconds and runs it over audio files as `transcription.transcribe_files` runs the decoders.

What a time means: one output frame of the network covers ``2 * hop_length`` samples (the features hop by ``hop_length`` = 160
samples and the first layer strides by 2), so frame f is reported as ``f * 2 * hop_length / sample_rate`` seconds.  That is a
NOMINAL time: the network's receptive field is wide (hundreds of milliseconds), a frame's logits depend on audio well before
and after its nominal position, and CTC training does not tie a character's peak to its acoustic onset.
"""
import contextlib
import json
import os
import sys
import time

from . import inference, transcription, vocabulary

HOP_LENGTH = 160                      # preprocessing.power_spectrogram_device / mfccs_device
TRANSCRIPT_SUFFIX = '.trans.txt'


def char_spans(ids, spans):
  """-> list of (character, first frame, end frame) for every id."""
  return [(vocabulary.id_to_letter(i), int(s[0]), int(s[1])) for i, s in zip(ids, spans)]


def word_runs(ids, space_id=vocabulary.SPACE_ID):
  """Words are maximal runs of ids other than space: -> list of (index of the word's first id, one past its last).  Leading,
  trailing and repeated spaces produce no words.  (The word_spans argument of st_ctc_word_conf_f32 is made of these.)"""
  runs, start = [], None
  for k, i in enumerate(list(ids) + [space_id]):
    if i != space_id:
      if start is None:
        start = k
    elif start is not None:
      runs.append((start, k))
      start = None
  return runs


def word_spans(ids, spans):
  """-> list of (word, first frame of its first character, end frame of its last character) for every word of `word_runs`."""
  ids = list(ids)
  return [(vocabulary.ids_to_sentence(ids[a:b]), int(spans[a][0]), int(spans[b - 1][1])) for a, b in word_runs(ids)]


WILDCARD = -1                         # engine_decode.WILDCARD (kept here so that this module imports without torch)
WILDCARD_TOKEN = '*'                  # how a transcript writes it: a word of its own, outside the vocabulary
WILDCARD_BIAS = -1.0                  # engine_decode.WILDCARD_BIAS: nats per frame, a guess that nobody has tuned on data


def wild_word_runs(ids, space_id=vocabulary.SPACE_ID):
  """`word_runs` for ids that may hold WILDCARD: a wildcard ends a word like a space and is never part of one
  -> (word runs, indices of the wildcards)."""
  ids = list(ids)
  runs = word_runs([space_id if i == WILDCARD else i for i in ids], space_id)
  return runs, [k for k, i in enumerate(ids) if i == WILDCARD]


def wild_word_spans(ids, spans):
  """`word_spans` for ids that may hold WILDCARD -> (words as (word, first frame, end frame), gaps as (first frame, end frame)
  of every wildcard: the stretches of audio the transcript leaves out)."""
  ids = list(ids)
  runs, stars = wild_word_runs(ids)
  return ([(vocabulary.ids_to_sentence(ids[a:b]), int(spans[a][0]), int(spans[b - 1][1])) for a, b in runs],
          [(int(spans[k][0]), int(spans[k][1])) for k in stars])


def word_fits(ids, spans, fit):
  """The per-label fit of `engine.align(fit=True)` grouped into the words of `wild_word_runs`: for every word the sum of its
  labels' fits over the frames those labels hold (blank frames inside the word belong to no label) -- nats per frame, 0 where
  the greedy reading of the audio spells the word, the more negative the less the audio says it."""
  runs, _ = wild_word_runs(ids)
  return [float(sum(float(fit[k]) for k in range(a, b))) / max(sum(int(spans[k][1]) - int(spans[k][0]) for k in range(a, b)), 1)
          for a, b in runs]


def confident_words(ids, confidence):
  """The JSON form without times: [{word, confidence}], ``confidence`` one probability per word of `word_runs`."""
  ids = list(ids)
  runs = word_runs(ids)
  if len(runs) != len(confidence):
    raise ValueError('{} confidences for {} words'.format(len(confidence), len(runs)))
  return [dict(word=vocabulary.ids_to_sentence(ids[a:b]), confidence=round(float(c), 6)) for (a, b), c in zip(runs, confidence)]


def frames_to_seconds(frame, sample_rate, hop_length=HOP_LENGTH, duration=None):
  """Nominal time of output frame ``frame`` (see the module text): ``frame * 2 * hop_length / sample_rate`` seconds, clipped
  to [0, duration] when the file's duration is given."""
  t = max(float(frame) * 2.0 * hop_length / float(sample_rate), 0.0)
  return t if duration is None else min(t, float(duration))


def concat_frame_seconds(frame_edges, segments, segment_frames, sample_rate, pad_seconds, duration, end=False):
  """Frame boundaries of the CONCATENATED output frames of a recording's segments (`align_files(segment=...)`) -> seconds in
  the file.  ``segments``: [{start, end}] in seconds of the file and time order; ``segment_frames``: the output frames each
  contributed (0 for one too short for the features); ``pad_seconds``: the zeros in front of each gathered segment.

  A boundary belongs to the segment of the frame it starts -- with ``end=True`` (one past the last frame of a span) to the
  segment of the frame before it, so the end of a word that closes a segment is not reported at the start of the next one --
  and is the segment's start, minus its pad, plus `frames_to_seconds` of the frame inside the segment, clipped to the file as
  `segmentation.stitch` clips.  The result is monotone over the whole file: a segment's times also stay on its own side of the
  middle of the gap to each neighbour, which only matters where a cut of an over-long utterance leaves no gap for the pads."""
  counts = [int(n) for n in segment_frames]
  if len(counts) != len(segments):
    raise ValueError('concat_frame_seconds: {} segments and {} frame counts'.format(len(segments), len(counts)))
  first = [0]
  for n in counts:
    first.append(first[-1] + n)
  used = [s for s, n in enumerate(counts) if n > 0]
  out = []
  for f in frame_edges:
    f = int(f)
    probe = f - 1 if end else f                      # the frame whose segment the boundary is taken in
    if not used or not 0 <= probe < first[-1]:
      raise ValueError('concat_frame_seconds: frame boundary {} outside the {} concatenated frames'.format(f, first[-1]))
    k = max(j for j, s in enumerate(used) if first[s] <= probe)
    s = used[k]
    lo = 0.0 if k == 0 else 0.5 * (float(segments[used[k - 1]]['end']) + float(segments[s]['start']))
    hi = float(duration) if k + 1 == len(used) else 0.5 * (float(segments[s]['end']) + float(segments[used[k + 1]]['start']))
    t = float(segments[s]['start']) - float(pad_seconds) + frames_to_seconds(f - first[s], sample_rate)
    out.append(min(max(t, lo, 0.0), hi, float(duration)))
  return out


def timed_words(ids, spans, sample_rate, duration=None, chars=False, confidence=None, concat=None, fit=None, gaps=False):
  """The JSON form: [{word, start, end}] in seconds (``chars``: of the single characters, as {char, start, end});
  ``confidence`` (one probability per word): each word also carries `confidence`.  ``concat``: (segments, segment_frames,
  pad_seconds) of an entry whose spans are in concatenated frames -- the times then come from `concat_frame_seconds`.
  Ids that hold WILDCARD: a wildcard is no word and no character; ``gaps=True`` returns their [{start, end}] instead.
  ``fit`` (the per-label fit of `engine.align`): each word also carries `fit` (`word_fits`)."""
  if concat is None:
    sec = end_sec = lambda f: round(frames_to_seconds(f, sample_rate, HOP_LENGTH, duration), 4)
  else:
    sec = lambda f: round(concat_frame_seconds([f], concat[0], concat[1], sample_rate, concat[2], duration)[0], 4)
    end_sec = lambda f: round(concat_frame_seconds([f], concat[0], concat[1], sample_rate, concat[2], duration, end=True)[0], 4)
  ids = list(ids)
  if gaps:
    return [dict(start=sec(a), end=end_sec(b)) for a, b in wild_word_spans(ids, spans)[1]]
  if chars:
    keep = [k for k, i in enumerate(ids) if i != WILDCARD]
    return [dict(char=c, start=sec(a), end=end_sec(b)) for c, a, b in char_spans([ids[k] for k in keep], [spans[k] for k in keep])]
  words = [dict(word=w, start=sec(a), end=end_sec(b))
           for w, a, b in (wild_word_spans(ids, spans)[0] if WILDCARD in ids else word_spans(ids, spans))]
  if fit is not None:
    for w, f in zip(words, word_fits(ids, spans, fit)):
      w['fit'] = round(f, 6)
  if confidence is not None:
    for w, c in zip(words, confident_words(ids, confidence)):
      w['confidence'] = c['confidence']
  return words


def read_transcripts(path):
  """A LibriSpeech-style transcript file, ``<id> <text>`` per line -> {id: text}; parsed as preprocessing.SpeechCorpusReader
  parses it (split at the first space), blank lines skipped, an id without text maps to ''."""
  out = {}
  with open(path, 'r') as f:
    for line in f:
      line = line.rstrip('\n').rstrip('\r')
      if not line.strip():
        continue
      parts = line.split(' ', 1)
      out[parts[0]] = parts[1] if len(parts) > 1 else ''
  return out


def find_transcripts(paths, transcripts_file=None):
  """{audio path: transcript text or None}: from ``transcripts_file`` when given, else from the *.trans.txt files in each audio
  file's own directory; the key is the file's stem."""
  tables = {}

  def table(directory):
    if directory not in tables:
      merged = {}
      try:
        names = sorted(n for n in os.listdir(directory or '.') if n.endswith(TRANSCRIPT_SUFFIX))
      except OSError:
        names = []
      for n in names:
        merged.update(read_transcripts(os.path.join(directory or '.', n)))
      tables[directory] = merged
    return tables[directory]

  given = read_transcripts(transcripts_file) if transcripts_file else None
  out = {}
  for p in paths:
    stem = os.path.splitext(os.path.basename(p))[0]
    out[p] = (given if given is not None else table(os.path.dirname(p))).get(stem)
  return out


def transcript_ids(text, wildcard=None, ends=False):
  """Ids of a transcript as the corpus reader makes them (vocabulary.sentence_to_ids after lower-casing); raises
  TranscriptionError for a character outside the vocabulary.

  ``wildcard`` (a token such as WILDCARD_TOKEN, outside the vocabulary): where it stands as a word of its own between spaces
  (or at an end of the text) it becomes the id WILDCARD, audio the transcript leaves out; anywhere else its characters are the
  vocabulary error they always were.  ``ends``: a wildcard and a space before the text and a space and a wildcard after it,
  unless the text has one there already -- a recording that opens and closes with words the transcript does not have."""
  if wildcard is not None:
    if not wildcard or ' ' in wildcard or all(c in vocabulary._TO_ID for c in wildcard.lower()):
      raise ValueError('the wildcard token must be a word outside the vocabulary, not {!r}'.format(wildcard))
    pieces = text.lower().split(' ')
    if ends and any(pieces):
      pieces = ([] if pieces[0] == wildcard.lower() else [wildcard.lower()]) + pieces + \
          ([] if pieces[-1] == wildcard.lower() else [wildcard.lower()])
    ids = []
    for k, piece in enumerate(pieces):
      ids += ([vocabulary.SPACE_ID] if k else []) + ([WILDCARD] if piece == wildcard.lower() else transcript_ids(piece))
    return ids
  ids = vocabulary.sentence_to_ids(text.lower())
  bad = sorted({ch for ch, i in zip(text.lower(), ids) if not 0 <= i < vocabulary.SIZE})
  if bad:
    raise transcription.TranscriptionError('transcript has characters outside the vocabulary: {}'.format(' '.join(map(repr, bad))))
  return ids


def align_files(engine, paths, transcripts, feature_type='power', sample_rate=22050, batch_size=1, timings=None, mask_padding=False,
                confidence=False, segment=None, wildcard=None, fit=False, ends=False, wildcard_bias=None):
  """Align audio files with their transcripts -> a list, in ``paths`` order, of dicts
  {path, seconds, sample_rate, text, ids, spans, score, frames, error}.  ``transcripts``: {path: text} (`find_transcripts`) or
  a list parallel to ``paths``; None = no transcript.  ``error`` is the message for a file that is unreadable, too short, has no
  transcript, or whose transcript does not fit its frames or the vocabulary (spans is None then); the other files go on.
  ``spans``: [L, 2] output frames per id; ``frames``: output frames of the utterance; ``sample_rate``: the rate the features
  were computed at (what `frames_to_seconds` needs).  Batch semantics as `transcription.transcribe_files`, ``mask_padding``
  included: with it the spans of a file do not depend on the batch it is in.  ``confidence=True``: every aligned entry gains
  ``confidence`` = {'log_prob': ln P(transcript), 'words': [probability per word of the transcript]} (`inference.align`).

  ``segment`` (a segmentation.SegmentOptions): long recordings.  Every file is cut at its silences on the device, the segments
  go through the network in batches, and the file's WHOLE transcript -- of any length, the limit of MAX_LABELS characters does
  not apply -- is aligned against the concatenated output frames of its segments (`inference.align_long`).  The entry gains
  ``segments`` ([{start, end}] in seconds of the file), ``segment_frames`` (the output frames of each; 0 for a segment too short
  for the features) and ``segment_pad`` (seconds of zeros in front of a gathered segment); ``spans`` are in concatenated frames,
  ``frames`` is their number, and `concat_frame_seconds` -- through `timed_words`, `result_json`, `print_words` -- maps them to
  seconds of the file.  Word confidences are not computed on this path.

  ``wildcard`` (a token, usually WILDCARD_TOKEN; ``ends=True`` implies that one): transcripts that leave audio out.  The token
  as a word of its own in a transcript becomes a wildcard label (`transcript_ids`; ``ids`` then holds WILDCARD there), which the
  best path gives the audio the text does not have, at ``wildcard_bias`` nats per frame (default WILDCARD_BIAS = -1.0, a guess
  that nobody has tuned on data).  ``ends=True`` puts one before and after every transcript: recordings that open and close with
  words the text lacks.  Aligned entries gain ``gaps``: [{start, end}] in seconds of the file, one per wildcard -- and, with
  ``fit=True``, ``fit`` (one float per id: `engine.align`) and ``word_fit`` (`word_fits`: nats per frame for every word; a very
  negative one marks text the audio does not say).  With and without ``segment``; not with ``confidence`` (the word-posterior
  lattices do not know the wildcard)."""
  if segment is not None and confidence:
    raise ValueError('align_files: word confidences are not available with segment')
  if ends and wildcard is None:
    wildcard = WILDCARD_TOKEN
  wild = wildcard is not None or bool(fit) or wildcard_bias is not None
  if wild and confidence:
    raise ValueError('align_files: word confidences are not available with a wildcard or the fit')
  if wild and wildcard_bias is None:
    wildcard_bias = WILDCARD_BIAS
  wild_args = dict(wildcard_bias=wildcard_bias, fit=True) if wild else {}
  texts = [transcripts.get(p) for p in paths] if isinstance(transcripts, dict) else list(transcripts)
  if len(texts) != len(paths):
    raise ValueError('align_files: {} paths and {} transcripts'.format(len(paths), len(texts)))
  results, signals, rates, ok = [], [], [], []
  t0 = time.perf_counter()
  for path, text in zip(paths, texts):
    entry = dict(path=path, seconds=None, sample_rate=None, text=None, ids=None, spans=None, score=None, frames=None, error=None)
    results.append(entry)
    try:
      samples, rate = transcription.load_native(path)
      entry['seconds'] = len(samples) / float(rate)
      entry['sample_rate'] = transcription._target_rate(rate, sample_rate)
      transcription.check_length(len(samples), rate, sample_rate, path)
      if text is None:
        raise transcription.TranscriptionError('{}: no transcript'.format(path))
      try:
        entry['ids'] = transcript_ids(text, wildcard, ends) if wildcard is not None else transcript_ids(text)
      except transcription.TranscriptionError as e:
        raise transcription.TranscriptionError('{}: {}'.format(path, e)) from e
      entry['text'] = text.lower()
      if segment is None and len(entry['ids']) > MAX_LABELS:
        raise transcription.TranscriptionError('{}: transcript of {} characters is too long to align (max {})'.format(
            path, len(entry['ids']), MAX_LABELS))
    except transcription.TranscriptionError as e:
      entry['error'] = str(e)
      continue
    signals.append(samples)
    rates.append(rate)
    ok.append(entry)
  t1 = time.perf_counter()
  if ok and segment is not None:
    from . import segmentation
    table, gathered, out_offsets = segmentation.segment_audio(signals, rates, segment, engine.device)
    feats = transcription.device_features_on_device(gathered, out_offsets, [int(rates[i]) for i in table[:, 0]], feature_type,
                                                    sample_rate) if len(table) else []
    t2 = time.perf_counter()
    for i, (entry, rate) in enumerate(zip(ok, rates)):
      rows = [s for s in range(len(table)) if table[s, 0] == i]
      entry['segments'] = [dict(start=int(table[s, 1]) / float(rate), end=int(table[s, 2]) / float(rate)) for s in rows]
      entry['segment_pad'] = segmentation.pad_samples(segment, rate) / float(rate)
      res = inference.align_long(engine, [feats[s] for s in rows if feats[s] is not None], entry['ids'],
                                 batch_size=batch_size, mask_padding=mask_padding, **wild_args)
      spans, score, status, frames = res[:4]
      frames = iter(frames)
      entry['segment_frames'] = [next(frames) if feats[s] is not None else 0 for s in rows]
      entry['frames'] = sum(entry['segment_frames'])
      if status != 0:
        entry['error'] = '{}: transcript does not fit: {} characters (repeats need a frame between them) on {} output frames'.format(
            entry['path'], len(entry['ids']), entry['frames'])
      else:
        entry['spans'], entry['score'] = spans, score
        if wild:
          _wild_entry(entry, res[-1], fit)
  elif ok:
    feats = transcription.device_features(signals, rates, feature_type, sample_rate, engine.device)
    t2 = time.perf_counter()
    res = inference.align(engine, feats, [e['ids'] for e in ok], batch_size=batch_size, mask_padding=mask_padding,
                          confidence=confidence, **wild_args)
    spans, scores, status = res[:3]
    if confidence:
      for entry, c in zip(ok, res[3]):
        if c is not None:
          entry['confidence'] = c
    for entry, f, sp, sc, st in zip(ok, feats, spans, scores, status):
      entry['frames'] = output_frames(f.shape[0])
      if st != 0:
        entry['error'] = '{}: transcript does not fit: {} characters (repeats need a frame between them) on {} output frames'.format(
            entry['path'], len(entry['ids']), entry['frames'])
      else:
        entry['spans'], entry['score'] = sp, sc
    if wild:
      for entry, f in zip(ok, res[-1]):
        if entry['spans'] is not None:
          _wild_entry(entry, f, fit)
  else:
    t2 = t1
  if timings is not None:
    timings.update(decode_host=t1 - t0, features=t2 - t1, align=time.perf_counter() - t2)
  return results


def _wild_entry(entry, fits, want_fit):
  """The ``gaps`` (and with ``want_fit`` the ``fit`` / ``word_fit``) of an aligned entry of `align_files`."""
  entry['gaps'] = timed_words(entry['ids'], entry['spans'], entry['sample_rate'], entry['seconds'], concat=concat_of(entry), gaps=True)
  if want_fit:
    entry['fit'] = [float(f) for f in fits]
    entry['word_fit'] = word_fits(entry['ids'], entry['spans'], fits)


MAX_LABELS = 511                      # engine_decode.MAX_ALIGN_LABELS (kept here so that this module imports without torch)


def output_frames(feature_frames):
  """Output frames of the network for ``feature_frames`` input frames: what the engine hands CTC and the decoders
  (sequence_lengths // 2, speech_model.py:74)."""
  return int(feature_frames) // 2


def concat_of(entry):
  """The ``concat`` argument of `timed_words` for an entry of `align_files(segment=...)`, None for any other."""
  if entry.get('segment_frames') is None:
    return None
  return entry['segments'], entry['segment_frames'], entry['segment_pad']


def result_json(entry, chars=False):
  """The --output line of an aligned (or transcribed with --timestamps) file."""
  rate, dur = entry['sample_rate'], entry['seconds']
  concat = concat_of(entry)
  out = dict(path=entry['path'], seconds=dur, text=entry['text'])
  if entry.get('score') is not None:
    out['score'] = entry['score']
    out['score_per_frame'] = entry['score'] / max(entry['frames'], 1)
  conf = entry.get('confidence')
  if conf is not None:
    out['log_prob'] = conf['log_prob']
  if entry.get('spans') is None:                       # transcribed with --confidence alone: words without times
    out['words'] = confident_words(entry['ids'], conf['words'])
    return out
  out['words'] = timed_words(entry['ids'], entry['spans'], rate, dur, confidence=conf['words'] if conf is not None else None,
                             concat=concat, fit=entry.get('fit'))
  if entry.get('gaps') is not None:
    out['gaps'] = entry['gaps']
  if chars:
    out['chars'] = timed_words(entry['ids'], entry['spans'], rate, dur, chars=True, concat=concat)
  if concat is not None:
    out['segments'] = [dict(start=round(g['start'], 4), end=round(g['end'], 4)) for g in entry['segments']]
  return out


def print_words(entry, file=None):
  """One line per word: path<TAB>start<TAB>end<TAB>word, and <TAB>confidence when the entry carries confidences (start and end
  are `-` for an entry without spans)."""
  conf = entry.get('confidence')
  if entry.get('spans') is None:
    words = confident_words(entry['ids'], conf['words'])
  else:
    words = timed_words(entry['ids'], entry['spans'], entry['sample_rate'], entry['seconds'],
                        confidence=conf['words'] if conf is not None else None, concat=concat_of(entry), fit=entry.get('fit'))
    # the gaps of a wildcard entry are lines of their own, in time order among the words: the token in the word's column
    words = sorted(words + [dict(g, word=WILDCARD_TOKEN) for g in entry.get('gaps') or []], key=lambda w: (w['start'], w['end']))
  for w in words:
    times = '{:.3f}\t{:.3f}'.format(w['start'], w['end']) if 'start' in w else '-\t-'
    tail = '\t{:.4f}'.format(w['confidence']) if conf is not None else ''
    if entry.get('fit') is not None:
      tail += '\t{:.4f}'.format(w['fit']) if 'fit' in w else '\t-'
    print('{}\t{}\t{}{}'.format(entry['path'], times, w['word'], tail), file=file or sys.stdout, flush=True)


def segment_options(flags):
  """The segmentation.SegmentOptions of `speecht-cli align --segment` (None without it).  The four flags are absent from the
  namespace unless given; their defaults are those of SegmentOptions, which are `transcribe`'s."""
  if not getattr(flags, 'segment', False):
    return None
  from . import segmentation
  d = segmentation.SegmentOptions()
  return segmentation.SegmentOptions(threshold=getattr(flags, 'segment_threshold', d.threshold),
                                     min_silence=getattr(flags, 'min_silence', d.min_silence),
                                     max_segment=getattr(flags, 'max_segment', d.max_segment))


def wildcard_options(flags):
  """The wildcard / fit arguments of `align_files` from `speecht-cli align --wildcard [TOKEN] --wildcard-ends --wildcard-bias X
  --fit` (the flags are absent from the namespace unless given; none of them: {} -- a `*` in a transcript stays a vocabulary
  error)."""
  token = getattr(flags, 'wildcard', None)
  ends = bool(getattr(flags, 'wildcard_ends', False))
  bias = getattr(flags, 'wildcard_bias', None)
  fit = bool(getattr(flags, 'fit', False))
  if token is None and (ends or bias is not None):
    token = WILDCARD_TOKEN
  if token is None and not fit:
    return {}
  return dict(wildcard=token, ends=ends, wildcard_bias=WILDCARD_BIAS if bias is None else float(bias), fit=fit)


def run_cli(flags):
  """`speecht-cli align`: prints path<TAB>start<TAB>end<TAB>word per word in input order (and JSON lines to --output); a file that
  cannot be aligned is reported on stderr and makes the exit status 1.  Creates no train / data / log directory."""
  from .speech_input import SingleInputLoader
  from .speech_model import Session, create_default_model
  paths = transcription.expand_paths(flags.paths)
  if not paths:
    print('align: no audio files found in {}'.format(' '.join(flags.paths)), file=sys.stderr)
    return 1
  try:
    transcripts = find_transcripts(paths, flags.transcripts)
  except OSError as e:
    print('align: cannot read transcripts: {}'.format(e), file=sys.stderr)
    return 1
  input_size = transcription.FEATURE_WIDTH[flags.feature_type]
  with contextlib.redirect_stdout(sys.stderr):          # stdout carries the word lines only
    model = create_default_model(flags, input_size, SingleInputLoader(input_size))
  segment = segment_options(flags)
  with Session(flags.device) as sess:
    with contextlib.redirect_stdout(sys.stderr):
      model.restore(sess, flags.run_train_dir)
    results = align_files(model.engine, paths, transcripts, flags.feature_type, flags.sample_rate, flags.batch_size,
                          mask_padding=bool(getattr(flags, 'mask_padding', False)),
                          confidence=bool(getattr(flags, 'confidence', False)), segment=segment, **wildcard_options(flags))
  out = open(flags.output, 'w') if flags.output else None
  status = 0
  try:
    for r in results:
      if r['error'] is not None:
        print('align: {}'.format(r['error']), file=sys.stderr)
        status = 1
        continue
      print_words(r)
      if out:
        out.write(json.dumps(result_json(r, chars=flags.chars)) + '\n')
  finally:
    if out:
      out.close()
  return status
