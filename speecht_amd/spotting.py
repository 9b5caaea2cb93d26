"""Keyword spotting: where in audio files somebody says given words or phrases -- `speecht-cli spot` and its Python API.

A character CTC model scores any character string against the frames directly (`engine.spot`, st_ctc_spot_f32; semantics and
tie rules: include/speecht_hip.h, tests/spot_oracle.py): a HIT of a keyword is a stretch of output frames read as a CTC
alignment of the keyword that begins on its first and ends on its last character, and its ``score`` is the log-likelihood
ratio of that reading against the best unconstrained (greedy) reading of the same frames -- the sum over the hit's frames of
(logit of the class read - largest logit), <= 0, and 0 exactly when the greedy decoder already spells the keyword there.  Unlike
a search in the transcripts it also finds occurrences the decoder spelled differently, and it ranks them.

``score_per_frame`` = score / frames of the hit is what ``threshold`` applies to: ln of the geometric-mean probability ratio
per frame.  The default, -0.69 = ln 0.5, is an interface default -- no trained model was available to tune it on.  Limits: the
score is a best path, not a posterior; a short keyword is also found inside longer words (add spaces to the phrase: " cat ");
under ``segment`` a keyword spoken across a cut is not found; times are nominal, as `alignment` explains.
"""
import contextlib
import json
import sys

import numpy as np

from . import alignment, inference, segmentation, transcription, vocabulary
from .transcription import TranscriptionError

MAX_LABELS = 511                      # engine_decode.MAX_SPOT_LABELS (kept here so that this module imports without torch)
DEFAULT_THRESHOLD = -0.69             # ln 0.5 per frame


def keyword_ids(text):
  """Ids of a keyword or phrase (vocabulary.sentence_to_ids after lower-casing); raises TranscriptionError for an empty one,
  one of more than MAX_LABELS ids or one with a character outside the vocabulary."""
  text = text.lower()
  ids = vocabulary.sentence_to_ids(text)
  if not ids:
    raise TranscriptionError('keyword is empty')
  bad = sorted({ch for ch, i in zip(text, ids) if not 0 <= i < vocabulary.SIZE})
  if bad:
    raise TranscriptionError('keyword {!r} has characters outside the vocabulary: {}'.format(text, ' '.join(map(repr, bad))))
  if len(ids) > MAX_LABELS:
    raise TranscriptionError('keyword of {} characters is too long (at most {})'.format(len(ids), MAX_LABELS))
  return ids


def read_keywords(path):
  """A keyword file: one keyword or phrase per line (its inner and outer spaces kept apart from the line end); blank lines and
  lines that begin with # are skipped, duplicates dropped in order."""
  out = []
  with open(path, 'r') as f:
    for line in f:
      line = line.rstrip('\n').rstrip('\r')
      if not line.strip() or line.lstrip().startswith('#'):
        continue
      if line.lower() not in out:
        out.append(line.lower())
  return out


def pick_hits(trace_score, trace_start, threshold):
  """Non-overlapping hits of one (utterance, keyword) from its trace (``engine.spot(trace=True)``) -> [(start, end, score)] in
  output frames, in order of acceptance.  The candidates are the frames with a finite end score, by score descending, then end
  descending; a candidate becomes a hit if its [start, end) overlaps no accepted hit and score / (end - start) >= threshold."""
  trace_score, trace_start = np.asarray(trace_score, dtype=np.float64), np.asarray(trace_start)
  ends = np.flatnonzero(np.isfinite(trace_score))
  order = ends[np.lexsort((-ends, -trace_score[ends]))]
  hits = []
  for t in order.tolist():
    score, start, end = float(trace_score[t]), int(trace_start[t]), t + 1
    if score / (end - start) >= threshold and all(end <= a or start >= b for a, b, _ in hits):
      hits.append((start, end, score))
  return hits


def _frame_hits(res, row, k, threshold, all_hits):
  """The hits of keyword k in utterance ``row`` of an `inference.spot` result, in output frames."""
  if all_hits:
    return pick_hits(res[3][row][k], res[4][row][k], threshold)
  score, (start, end) = float(res[0][row, k]), res[1][row, k]
  if np.isfinite(score) and score / (end - start) >= threshold:
    return [(int(start), int(end), score)]
  return []


def _timed(keyword, start, end, score, rate, duration):
  sec = lambda f: round(alignment.frames_to_seconds(f, rate, alignment.HOP_LENGTH, duration), 4)
  return dict(keyword=keyword, start=sec(start), end=sec(end), score=score, score_per_frame=score / (end - start))


def _best_per_keyword(hits, keywords):
  """Of several segments' best hits the best per keyword: the largest score, the earlier one among equals."""
  best = {}
  for h in hits:
    if h['keyword'] not in best or h['score'] > best[h['keyword']]['score']:
      best[h['keyword']] = h
  return [best[k] for k in keywords if k in best]


def _without_overlaps(hits, keywords):
  """Hits of several segments in file time: the padded ends of neighbouring segments may cover the same audio, so of two hits of
  one keyword that overlap the better one stays (by score descending, then end descending, as `pick_hits`)."""
  kept = []
  for k in keywords:
    mine = []
    for h in sorted((h for h in hits if h['keyword'] == k), key=lambda h: (-h['score'], -h['end'])):
      if all(h['end'] <= o['start'] or h['start'] >= o['end'] for o in mine):
        mine.append(h)
    kept += mine
  return kept


def spot_audio(engine, signals, rates, keywords, feature_type='power', sample_rate=22050, batch_size=1, mask_padding=False,
               threshold=DEFAULT_THRESHOLD, all_hits=False, segment=None):
  """Find keywords (strings) in float32 mono signals at the given source rates -> per signal a list of hits
  {keyword, start, end (seconds in the signal), score, score_per_frame}, by start time.  Default: the best hit of every keyword
  in the signal, if its score_per_frame reaches ``threshold``; ``all_hits``: every non-overlapping hit that does (`pick_hits`).

  Features and batches as transcription.transcribe_audio (``batch_size=1`` by default, for the same reason; ``mask_padding``).
  ``segment`` (a segmentation.SegmentOptions): every signal is cut into utterances at its silences on the device, the keywords
  are searched per utterance and the hits reported in the signal's time; a keyword spoken across a cut is not found."""
  keywords = list(keywords)
  ids = [keyword_ids(k) for k in keywords]
  out = [[] for _ in signals]
  if not len(signals) or not keywords:
    return out
  if segment is None:
    feats = transcription.device_features(signals, rates, feature_type, sample_rate, engine.device)
    res = inference.spot(engine, feats, ids, batch_size=batch_size, mask_padding=mask_padding, trace=all_hits)
    for i, (signal, rate) in enumerate(zip(signals, rates)):
      target, duration = transcription._target_rate(int(rate), sample_rate), len(signal) / float(rate)
      for k, keyword in enumerate(keywords):
        out[i] += [_timed(keyword, a, e, s, target, duration) for a, e, s in _frame_hits(res, i, k, threshold, all_hits)]
  else:
    table, gathered, out_offsets = segmentation.segment_audio(signals, rates, segment, engine.device)
    if len(table):
      seg_rates = [int(rates[i]) for i in table[:, 0]]
      feats = transcription.device_features_on_device(gathered, out_offsets, seg_rates, feature_type, sample_rate)
      ok = [s for s, f in enumerate(feats) if f is not None]          # (a segment too short for the features holds no hit)
      res = inference.spot(engine, [feats[s] for s in ok], ids, batch_size=batch_size, mask_padding=mask_padding, trace=all_hits)
      for row, s in enumerate(ok):
        i, a, _ = table[s].tolist()
        rate = float(rates[i])
        target = transcription._target_rate(int(rates[i]), sample_rate)
        inside = []
        for k, keyword in enumerate(keywords):
          inside += [_timed(keyword, f0, f1, sc, target, (out_offsets[s + 1] - out_offsets[s]) / rate)
                     for f0, f1, sc in _frame_hits(res, row, k, threshold, all_hits)]
        out[i] += segmentation.stitch(inside, a / rate, segmentation.pad_samples(segment, rates[i]) / rate, len(signals[i]) / rate)
      out = [_without_overlaps(hits, keywords) if all_hits else _best_per_keyword(hits, keywords) for hits in out]
  order = {k: n for n, k in enumerate(keywords)}
  return [sorted(hits, key=lambda h: (h['start'], h['end'], order[h['keyword']])) for hits in out]


def spot_files(engine, paths, keywords, feature_type='power', sample_rate=22050, batch_size=1, mask_padding=False,
               threshold=DEFAULT_THRESHOLD, all_hits=False, segment=None):
  """Find keywords (strings) in audio files (.flac, 16-bit .wav, .npy taken as 16 kHz) -> a list, in ``paths`` order, of dicts
  {path, seconds, error, hits}: ``error`` is the message for a file that cannot be read or is too short (its hits are None);
  the other files are searched as `spot_audio` does (same arguments).  A keyword that cannot be searched (empty, too long, a
  character outside the vocabulary) raises TranscriptionError before any file is read."""
  keywords = list(keywords)
  for k in keywords:
    keyword_ids(k)
  results, signals, rates, ok = [], [], [], []
  for path in paths:
    entry = dict(path=path, seconds=None, error=None, hits=None)
    results.append(entry)
    try:
      samples, rate = transcription.load_native(path)
      entry['seconds'] = len(samples) / float(rate)
      transcription.check_length(len(samples), rate, sample_rate, path)
    except TranscriptionError as e:
      entry['error'] = str(e)
      continue
    signals.append(samples)
    rates.append(rate)
    ok.append(entry)
  if ok:
    hits = spot_audio(engine, signals, rates, keywords, feature_type, sample_rate, batch_size, mask_padding, threshold, all_hits,
                      segment)
    for entry, h in zip(ok, hits):
      entry['hits'] = h
  return results


def print_hits(entry, file=None):
  """One line per hit: path<TAB>start<TAB>end<TAB>keyword<TAB>score<TAB>score_per_frame."""
  for h in entry['hits']:
    print('{}\t{:.3f}\t{:.3f}\t{}\t{:.4f}\t{:.4f}'.format(entry['path'], h['start'], h['end'], h['keyword'], h['score'],
                                                            h['score_per_frame']), file=file or sys.stdout, flush=True)


def result_json(entry):
  """The --output line of a searched file."""
  return dict(path=entry['path'], seconds=entry['seconds'], hits=entry['hits'])


def run_cli(flags):
  """`speecht-cli spot`: prints path<TAB>start<TAB>end<TAB>keyword<TAB>score<TAB>score_per_frame per hit, in file order and then by
  start (and JSON lines to --output); a file that cannot be read is reported on stderr and makes the exit status 1.  Creates no
  train / data / log directory."""
  from .speech_input import SingleInputLoader
  from .speech_model import Session, create_default_model
  paths = transcription.expand_paths(flags.paths)
  if not paths:
    print('spot: no audio files found in {}'.format(' '.join(flags.paths)), file=sys.stderr)
    return 1
  try:
    keywords = read_keywords(flags.keywords) if flags.keywords else []
    for k in flags.keyword or []:
      if k.lower() not in keywords:
        keywords.append(k.lower())
    if not keywords:
      raise TranscriptionError('no keywords given')
    for k in keywords:
      keyword_ids(k)
  except (OSError, TranscriptionError) as e:
    print('spot: {}'.format(e), file=sys.stderr)
    return 1
  input_size = transcription.FEATURE_WIDTH[flags.feature_type]
  with contextlib.redirect_stdout(sys.stderr):          # stdout carries the hit lines only
    model = create_default_model(flags, input_size, SingleInputLoader(input_size))
  segment = None
  if getattr(flags, 'segment', False):
    segment = segmentation.SegmentOptions(threshold=flags.segment_threshold, min_silence=flags.min_silence,
                                          max_segment=flags.max_segment)
  with Session(flags.device) as sess:
    with contextlib.redirect_stdout(sys.stderr):
      model.restore(sess, flags.run_train_dir)
    results = spot_files(model.engine, paths, keywords, flags.feature_type, flags.sample_rate, flags.batch_size,
                         mask_padding=bool(getattr(flags, 'mask_padding', False)), threshold=flags.threshold,
                         all_hits=bool(getattr(flags, 'all_hits', False)), segment=segment)
  out = open(flags.output, 'w') if flags.output else None
  status = 0
  try:
    for r in results:
      if r['error'] is not None:
        print('spot: {}'.format(r['error']), file=sys.stderr)
        status = 1
        continue
      print_hits(r)
      if out:
        out.write(json.dumps(result_json(r)) + '\n')
  finally:
    if out:
      out.close()
  return status
