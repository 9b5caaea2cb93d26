"""Streaming recognition: a stateful, chunked forward pass with live partial transcripts (csrc/conv_stream.hip).

Every layer's SAME padding has a left part that does not depend on the utterance's length, so an output frame is final as soon
as its right context has arrived: the first logits row after 99 input frames (0.99 s at the 10 ms hop), a steady lag of 49
output frames.  Each layer keeps a window of recent input frames per stream; a step runs the eleven products over the frames
that have become ready in all named streams at once, moves the windows on and decodes greedily across the step boundary.

The index arithmetic below is the Python twin of csrc/stream_map.h: pure functions of the layer list ``(width, stride)`` and a
stream's counters.  The counters depend only on how many frames were fed, so the host keeps them and sizes every step
(`plan`) before anything is launched; the device gets them as one small table per step.  Only the decoder's state lives on
the device.

A stream's logits are bit-identical however its audio was cut into chunks and whatever the other streams were doing: the
product kernel cuts every layer's reduction into slices that depend on the layer's shape only and sums them in slice order.
The arithmetic is fp32 (the engine's packed fp32 masters) whatever mode the engine trains in.

With ``beam=StreamBeam(...)`` a step also advances a CTC prefix beam search per stream -- LM-free or scored by a word n-gram
model, the searches of `transcribe` -- whose state (the live beam set, its LM states, the node pool) stays on the device between
steps.  A chunked search is the whole-utterance search: after `finish` the hypothesis and its log-probability are what
``engine.beam_search_decode`` / ``lm_beam_search_decode`` return on the stream's logits, bit for bit and however the audio was cut.
Before that a step reports the best hypothesis so far and how many of its leading ids are final (the common prefix of all live
entries).  Such a stream can decode ``StreamBeam.max_seconds`` of audio: its node pool is sized when the recogniser is built.
``StreamBeam(hotwords=...)`` biases that search towards phrases as ``transcribe(hotwords=)`` does (speecht_amd/hotwords.py), with one
phrase set for all streams or -- `hotwords.HotwordSets`, ``open(hotwords=k)`` -- a set per stream; `finish` then returns what
``engine.beam_search_decode_nbest(1, ..., hotwords=)`` returns on the stream's logits with the stream's set.

With ``endpoint=Endpointing(...)`` the device also cuts every stream into utterances (csrc/stream_endpoint.hip): once silence has
followed speech, or an utterance has reached its longest length, the step hands back a final -- the offline decoder's result on
that utterance's rows alone -- and the decoders start again, so a stream may run for any length on a node pool of one utterance.
The logits are the same with and without it; the rule is a pure function of a stream's logits rows (tests/endpoint_oracle.py).

With ``words=FinalWords(...)`` (and endpointing) every final also carries its words' times and confidences: each pass copies its logits
rows into a ring per stream (csrc/stream_words.hip), and the pass that closes an utterance runs the lattices of ``engine.align`` and
``engine.word_confidence`` on the utterance's rows in that ring -- what those calls return on the rows alone, bit for bit.

With ``beam=StreamBeam(nbest=N)`` every final also carries the N best hypotheses of its search -- `Utterance.nbest`, or
`StepResult.nbest` after `finish` without endpointing: the list the whole-utterance N-best searches return on the utterance's rows
alone, bit for bit, written by the read-out kernel into a compact arena that only a pass with finals copies
(st_ctc_beam_stream_read_nbest / _step_pieces_nbest, `nbest.read_arena`) -- and ``rescore=`` re-ranks the lists of a pass together
under a second language model before the words are aligned: two-pass decoding, as ``transcribe(nbest=, rescore=)`` does offline.

With ``spot=StreamSpotter(...)`` every step also tells which of the given words and phrases have just been said in each stream
(csrc/ctc_spot_stream.hip): the lattices of `speecht-cli spot` carried across steps, all keywords of a stream packed into a few
waves, and a causal rule that lets a hit go once nothing better can replace it (include/speecht_hip.h,
tests/spot_stream_oracle.py).  It runs on the stream's rows as they are: decoding and endpointing neither see nor reset it.

A model trained by this project expects 22 050 Hz audio (`preprocessing.LIBROSA_RATE`); live audio rarely has that rate.
`StreamingResampler` brings streams of any source rates to the model's as the samples arrive (csrc/resample_stream.hip): band-limited
interpolation has finite support, so an output sample is final (L + 1) / source_rate seconds after its time, and the streamed samples
are the offline resampler's of the whole signal, bit for bit.  `StreamingFeatures(model_rate, ..., source_rate=)` puts it in front of
the mel kernel without a trip through the host, `stream_audio(..., model_rate=)` and `speecht-cli stream --model-rate` use that, and
the seconds of endpointing, spotting, the beam's pool and the words' times then count frames of hop / model_rate seconds
(``frame_rate``) instead of assuming 10 ms.

On the host every option owns its part of a pass (`_EndpointPart`, `_BeamPart`, `_WordsPart`, `_SpotPart`, `_FollowPart`: state,
launches, read-out), and `StepLayout` alone says where each of them finds its results in the step's one copy back.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import call


class StreamError(ValueError):
  """A request the recogniser refuses; nothing was launched and no stream's state has changed.  (One exception: a beam search
  whose read-out gave up -- more labels still open than ``max_tail`` -- is reported after its step; that stream can only be
  closed, the others go on, and their results of the step are in the exception's ``result``.)"""


# ---- index arithmetic (csrc/stream_map.h) ---------------------------------------------------------------------------------

def pad_left(width, stride):
  return (width - stride) // 2 if width > stride else 0


def pad_left_fixed(width, stride):
  """True when SAME padding's left part is the same for every utterance length."""
  return stride >= 1 and width >= stride and (width - stride) // 2 == (width - 1) // 2


def ready_count(n, width, stride, finished):
  """Output frames that are final after ``n`` input frames."""
  if n <= 0:
    return 0
  if finished:
    return -(-n // stride)
  last = n - width + pad_left(width, stride)
  return 0 if last < 0 else last // stride + 1


def emit_count(n, e, width, stride, finished):
  return max(ready_count(n, width, stride, finished) - e, 0)


def retain_from(e, width, stride):
  """First absolute input frame still needed once ``e`` outputs are out (negative indices are padding, never stored)."""
  return max(e * stride - pad_left(width, stride), 0)


def decode_limit(total_input_frames):
  """Logits rows greedy decoding takes: the engine decodes ``seq_len // 2`` rows, so an odd length's last row is not decoded."""
  return total_input_frames // 2


def plan(layers, n, e, new, finished):
  """One step of one stream.  ``layers``: [(width, stride), ...]; ``n`` / ``e``: input frames received / output frames emitted
  per layer before the step; ``new`` input frames arrive at the first layer; ``finished``: flush with the right padding.
  Returns ``(steps, n_after, e_after)``, ``steps[l] = (first, count, base, n, new_base)``: layer l emits output frames
  ``first ... first + count - 1``, its window starts at absolute input frame ``base`` during the step and holds frames up to
  ``n``; afterwards it starts at ``new_base``."""
  steps, n_after, e_after = [], [], []
  for (width, stride), n_l, e_l in zip(layers, n, e):
    n_l += new
    count = emit_count(n_l, e_l, width, stride, finished)
    steps.append((e_l, count, retain_from(e_l, width, stride), n_l, retain_from(e_l + count, width, stride)))
    n_after.append(n_l)
    e_after.append(e_l + count)
    new = count
  return steps, n_after, e_after


def plan_many(layers, n, e, new, finished):
  """`plan` for k streams at once: ``n`` / ``e`` int arrays [k, layers], ``new`` [k], ``finished`` bool [k] -> int arrays [k, layers]
  ``(first, count, base, n_after, new_base)``.  The session sizes a step with this one; the tests hold it to `plan`."""
  n, e = np.asarray(n, dtype=np.int64), np.asarray(e, dtype=np.int64)
  add, fin = np.asarray(new, dtype=np.int64), np.asarray(finished, dtype=bool)
  first, count, base, n_after, new_base = (np.zeros_like(n) for _ in range(5))
  for l, (width, stride) in enumerate(layers):
    pl = pad_left(width, stride)
    n_l = n[:, l] + add
    last = n_l - width + pl
    ready = np.where(fin, -(-n_l // stride), np.where(last < 0, 0, last // stride + 1))
    ready = np.where(n_l <= 0, 0, ready)
    c = np.maximum(ready - e[:, l], 0)
    first[:, l], count[:, l], n_after[:, l] = e[:, l], c, n_l
    base[:, l] = np.maximum(e[:, l] * stride - pl, 0)
    new_base[:, l] = np.maximum((e[:, l] + c) * stride - pl, 0)
    add = c
  return first, count, base, n_after, new_base


def max_new_frames(layers, max_chunk):
  """Upper bound of the frames each layer can receive in one step (``[l]``) and of the rows the last layer can emit (``[-1]``):
  a layer that receives m frames emits at most ceil((m + width - pad_left + stride - 2) / stride), the flush at `finish` included."""
  out = [int(max_chunk)]
  for width, stride in layers:
    out.append(max(-(-(out[-1] + width - pad_left(width, stride) + stride - 2) // stride), 1))
  return out


def first_row_after(layers):
  """Input frames after which the first logits row is final, and the steady lag in output frames."""
  n = 0
  while True:
    n += 1
    r = n
    for width, stride in layers:
      r = ready_count(r, width, stride, False)
    if r > 0:
      break
  total = 1
  for _, stride in layers:
    total *= stride
  return n, -(-n // total) - 1


# ---- the session ----------------------------------------------------------------------------------------------------------

def seconds_to_frames(seconds, total_stride, frame_rate=None):
  """Seconds -> output frames of a model whose layers' strides multiply to ``total_stride``, rounded up and at least 1.  ``frame_rate``:
  feature frames per second, sample rate / hop (137.8125 for 22 050 Hz); None: 100, the 10 ms hop of 16 kHz audio, a guess."""
  return max(int(np.ceil(seconds * (100.0 if frame_rate is None else float(frame_rate)) / total_stride - 1e-9)), 1)


class StreamBeam:
  """The beam search of a `StreamingRecognizer` (st_ctc_beam_stream_step / _read): the prefix beam search of
  ``engine.beam_search_decode`` -- with ``lm`` (a `language_model.LanguageModel` or the path of an ARPA file) that of
  ``engine.lm_beam_search_decode`` -- carried across steps, with those methods' defaults: beam 16 on the logits without a model,
  beam 100 on log10(softmax + 1e-8) with one.  ``max_seconds`` sizes every stream's node pool (8 B x beam x 50 output frames per
  second of audio); ``max_tail`` is the longest run of not yet final labels a step can report.  ``hotwords``: the search biased
  towards phrases, as ``engine.beam_search_decode_nbest(..., hotwords=)`` is (st_ctc_beam_stream_step_bias / _read_bias /
  _step_pieces_bias) -- a `hotwords.Hotwords`, which every stream then uses, or a `hotwords.HotwordSets`, of which every stream
  names one when it is opened (`StreamingRecognizer.open(hotwords=index)`; set 0, the empty one, by default).

  ``nbest`` (an int in 1..beam_width): every final -- an `Utterance` of an endpointed stream, or what `finish` returns -- also carries
  the N best hypotheses of its search (st_ctc_beam_stream_read_nbest / _step_pieces_nbest): the list
  ``engine.beam_search_decode_nbest`` / ``lm_beam_search_decode_nbest`` returns on the utterance's rows alone, bit for bit, with the
  parts `nbest.components` attaches.  ``rescore`` (needs ``nbest``): the dict of `inference.transcribe` -- 'language_model' (a
  `LanguageModel` or a path) and optionally 'lm_weight', 'word_count_weight', 'valid_word_count_weight', with the defaults there --
  re-ranks every list under that model (`nbest.rescored`), and the final's ids are then the re-ranked first hypothesis's.
  ``nbest_words``: the capacity, in int32 words, of the arena the device writes a step's lists into (default: one final per stream
  with ``nbest`` tails of ``max_tail`` labels); lists beyond it are lost and counted (`StepResult.nbest_lost`)."""

  def __init__(self, beam_width=None, lm=None, lm_weight=0.8, word_count_weight=0.0, valid_word_count_weight=2.3, oov_score=-1000.0,
               input_transform='default', max_seconds=120.0, max_tail=256, hotwords=None, nbest=None, rescore=None, nbest_words=None):
    # (the list options first: a bad combination is refused before a model is loaded)
    width = int(beam_width) if beam_width else (100 if lm is not None else 16)
    if nbest is None:
      if rescore is not None:
        raise StreamError('rescore applies to N-best lists (nbest=N)')
      if nbest_words is not None:
        raise StreamError('nbest_words sizes the arena of N-best lists (nbest=N)')
    else:
      if not isinstance(nbest, (int, np.integer)) or isinstance(nbest, bool) or not 1 <= nbest <= width:
        raise StreamError('nbest must be an integer in 1..beam_width ({}), got {!r}'.format(width, nbest))
      if nbest_words is not None and (not isinstance(nbest_words, (int, np.integer)) or isinstance(nbest_words, bool)
                                      or not 0 <= nbest_words < 2 ** 31):
        raise StreamError('nbest_words must be a number of int32 words, got {!r}'.format(nbest_words))
      if rescore is not None:
        if not isinstance(rescore, dict) or rescore.get('language_model') is None:
          raise StreamError("rescore needs a 'language_model'")
        unknown = set(rescore) - {'language_model', 'lm_weight', 'word_count_weight', 'valid_word_count_weight'}
        if unknown:
          raise StreamError('rescore: unknown keys {}'.format(sorted(unknown)))
    self.nbest = None if nbest is None else int(nbest)
    self.nbest_words = None if nbest_words is None else int(nbest_words)
    self.rescore = None
    if rescore is not None:
      from .language_model import LanguageModel
      lm2 = rescore['language_model']
      shared = (float(word_count_weight), float(valid_word_count_weight)) if lm is not None else (0.0, 0.0)
      self.rescore = dict(language_model=lm2 if isinstance(lm2, LanguageModel) else LanguageModel.load(lm2),
                          lm_weight=float(rescore.get('lm_weight', lm_weight)),
                          word_count_weight=float(rescore.get('word_count_weight', shared[0])),
                          valid_word_count_weight=float(rescore.get('valid_word_count_weight', shared[1])))
    self.hotwords, self.default_set = None, 0
    if hotwords is not None:
      from .hotwords import Hotwords, HotwordSets
      if isinstance(hotwords, Hotwords):
        self.hotwords, self.default_set = HotwordSets([hotwords]), 1
      elif isinstance(hotwords, HotwordSets):
        self.hotwords = hotwords
      else:
        raise StreamError('hotwords must be a Hotwords or a HotwordSets, got {!r}'.format(type(hotwords).__name__))
    if isinstance(lm, str):
      from .language_model import LanguageModel
      lm = LanguageModel.load(lm)
    self.lm = lm
    self.beam_width = int(beam_width) if beam_width else (100 if lm is not None else 16)
    if input_transform == 'default':
      input_transform = 'log10_softmax' if lm is not None else None
    self.input_transform = input_transform
    self.lm_weight, self.word_count_weight = float(lm_weight), float(word_count_weight)
    self.valid_word_count_weight, self.oov_score = float(valid_word_count_weight), float(oov_score)
    self.max_seconds, self.max_tail = float(max_seconds), int(max_tail)
    if not 1 <= self.beam_width <= 128:
      raise StreamError('beam width 1..128 supported, got {}'.format(self.beam_width))
    if self.max_seconds <= 0 or self.max_tail < 1:
      raise StreamError('max_seconds and max_tail must be positive')

  def arena_words(self, max_streams):
    """The int32 words of the arena of a pass's lists: ``nbest_words``, or by default one final per stream, ``nbest`` hypotheses with
    tails of ``max_tail`` labels each.  None without lists."""
    if self.nbest is None:
      return None
    from .nbest import ARENA_HEADER
    words = max_streams * (ARENA_HEADER + self.nbest * (2 + self.max_tail)) if self.nbest_words is None else self.nbest_words
    if words >= 2 ** 31:
      raise StreamError('the arena of the N-best lists would hold {} words (nbest_words)'.format(words))
    return words


class Endpointing:
  """Endpointing of a `StreamingRecognizer` (st_ctc_greedy_endpoint_stream; the rule: include/speecht_hip.h, tests/endpoint_oracle.py):
  the device closes an utterance once ``silence`` seconds of rows whose best class is the blank or the space have followed speech, or
  when it reaches ``max_utterance`` seconds, and drops ``lead`` seconds that hold no speech at all; the decoders start again after
  each.  A beam search's node pool then holds ``max_utterance`` seconds, whatever the stream's length.  ``space_id``: the class that
  counts as silent beside the blank ('auto': 27 with the 29 classes a-z ' space blank, none otherwise; -1: none).  The 0.5 s default
  of ``silence`` is a guess, not tuned on data."""

  KINDS = {1: 'silence', 2: 'length', 4: 'end'}

  def __init__(self, silence=0.5, lead=1.0, max_utterance=30.0, space_id='auto'):
    self.silence, self.lead, self.max_utterance = float(silence), float(lead), float(max_utterance)
    for name in ('silence', 'lead', 'max_utterance'):
      v = getattr(self, name)
      if not (np.isfinite(v) and v > 0):
        raise StreamError('endpointing: {} must be a positive number of seconds, got {!r}'.format(name, v))
    if self.lead > self.max_utterance:
      raise StreamError('endpointing: lead ({} s) must not exceed max_utterance ({} s): a stretch without speech could outgrow the '
                        'node pool'.format(self.lead, self.max_utterance))
    if space_id != 'auto' and (not isinstance(space_id, (int, np.integer)) or space_id < -1):
      raise StreamError('endpointing: space_id must be \'auto\', -1 or a class index, got {!r}'.format(space_id))
    self.space_id = space_id

  def frames(self, total_stride, num_classes, frame_rate=None):
    """Seconds -> output frames of a model whose layers' strides multiply to ``total_stride``:
    ``(silence_frames, lead_frames, max_frames, space_id)``, each count rounded up and at least 1 (`seconds_to_frames`).
    ``frame_rate``: feature frames per second."""
    R, L, M = (seconds_to_frames(v, total_stride, frame_rate) for v in (self.silence, self.lead, self.max_utterance))
    space = (27 if num_classes == 29 else -1) if self.space_id == 'auto' else int(self.space_id)
    if space >= num_classes:
      raise StreamError('endpointing: space_id {} is no class of a model with {} classes'.format(space, num_classes))
    return R, L, max(M, L), space


class FinalWords:
  """Word times and confidences for the finals of an endpointed `StreamingRecognizer` (st_stream_keep_f32, st_ctc_align_ring_f32,
  st_ctc_word_conf_ring_f32; include/speecht_hip.h): the recogniser keeps every stream's recent logits rows in a ring on the device,
  and the pass that closes an utterance runs the lattices of ``engine.align`` (``timestamps``) and ``engine.word_confidence``
  (``confidence``) on the utterance's rows with the final's ids.  What a final then carries is what those offline calls return on its
  rows alone, bit for bit, however the audio was cut into steps.  ``confidence`` needs a space class -- the endpointing's
  ``space_id``, which must be the vocabulary's, whose helpers cut the ids into words -- and at most 30 classes.  One setting serves all
  streams."""

  def __init__(self, timestamps=True, confidence=False):
    self.timestamps, self.confidence = bool(timestamps), bool(confidence)
    if not (self.timestamps or self.confidence):
      raise StreamError('words: neither timestamps nor confidence is asked for')

  def check(self, endpoint, num_classes, space_id):
    """Refuses what the recogniser cannot serve; ``space_id``: the endpointing's, resolved for ``num_classes`` (-1: none)."""
    from . import vocabulary
    if endpoint is None:
      raise StreamError('words: word times and confidences need endpoint=Endpointing(...): the utterance of a stream that is not '
                        'endpointed has no bound')
    if not 2 <= num_classes <= 32:
      raise StreamError('words: the alignment supports 2..32 classes, the engine has {}'.format(num_classes))
    if self.confidence:
      if space_id < 0:
        raise StreamError('words: confidence needs a space class, the endpointing names none (space_id)')
      if num_classes > 30:
        raise StreamError('words: confidence supports at most 30 classes, the engine has {}'.format(num_classes))
      if space_id != vocabulary.SPACE_ID:
        raise StreamError('words: confidence cuts words at the vocabulary\'s space ({}), the endpointing names {}'.format(
            vocabulary.SPACE_ID, space_id))


def final_jobs(finals, space_id=None, max_labels=511):
  """The host's table for the lattices of a pass's finals.  ``finals``: [(stream, start_frame, end_frame, ids)] in any order; those with
  1 .. ``max_labels`` ids become jobs, in order.  -> dict: ``index`` (position in ``finals`` of every job), ``jobs`` int32 [n, 3] =
  {stream, u0, rows}, ``ids`` / ``offsets`` (the labels, CSR over the jobs), ``word_spans`` int32 [W, 3] = {job, first id, one past the
  last} from `alignment.word_runs` (empty without ``space_id``), ``words`` (how many words each job has), ``max_len`` and ``max_rows``
  (the longest label and utterance among the jobs)."""
  from . import alignment
  index = [i for i, f in enumerate(finals) if 1 <= len(f[3]) <= max_labels]
  jobs = np.asarray([(finals[i][0], finals[i][1], finals[i][2] - finals[i][1]) for i in index], dtype=np.int32).reshape(-1, 3)
  labels = [list(finals[i][3]) for i in index]
  offsets = np.zeros(len(index) + 1, dtype=np.int32)
  offsets[1:] = np.cumsum([len(l) for l in labels])
  runs = [alignment.word_runs(l, space_id) if space_id is not None else [] for l in labels]
  return dict(index=index, jobs=jobs, ids=np.asarray([i for l in labels for i in l], dtype=np.int32), offsets=offsets,
              word_spans=np.asarray([(j, a, e) for j, r in enumerate(runs) for a, e in r], dtype=np.int32).reshape(-1, 3),
              words=[len(r) for r in runs], max_len=max([len(l) for l in labels] + [0]),
              max_rows=int(jobs[:, 2].max()) if len(index) else 0)


class Utterance:
  """A final of an endpointed stream: utterance ``index`` of its stream, closed by ``kind`` ('silence', 'length' or, at `finish`, 'end'),
  the logits rows ``[start_frame, end_frame)`` with speech from ``first_speech`` to ``last_speech``.  ``ids``: the beam search's result on
  those rows alone with its log-probability ``logp`` -- what the whole-utterance search returns on them -- or, without a beam search,
  the greedy ids; ``greedy_ids`` and ``score`` (the negative sum of the chosen logits) are the greedy decoder's either way.

  With ``words=FinalWords(...)``: ``spans`` ([L, 2] int32, the first row and one past the last row of every id, relative to
  ``start_frame``) and ``align_score`` -- what ``engine.align`` returns on the utterance's rows --, ``confidence`` ({'log_prob', 'words'}
  as `inference.transcribe(confidence=True)` shapes it) and ``words``, a list of {word, start, end[, confidence]} with times in seconds
  from the stream's start (without ``timestamps``: {word, confidence}).  A final without ids has ``words == []`` and empty spans; one
  with more than ``engine_decode.MAX_ALIGN_LABELS`` ids, or whose ids do not fit its rows (a beam hypothesis with adjacent repeats
  can do that), has None for all four, as offline.  Without ``words`` -- and a field its `FinalWords` does not ask for -- None.

  With ``StreamBeam(nbest=N)``: ``nbest``, the list of `nbest.Hypothesis` of the search on the utterance's rows, best first, with the
  parts `nbest.components` attaches -- re-ranked (`nbest.rescored`) with ``StreamBeam(rescore=...)``, and ``ids`` / ``logp`` are then
  its first hypothesis's.  None without the option, and when the list did not fit the arena (`StepResult.nbest_lost`)."""
  __slots__ = ('index', 'kind', 'start_frame', 'end_frame', 'first_speech', 'last_speech', 'ids', 'logp', 'greedy_ids', 'score',
               'spans', 'align_score', 'confidence', 'words', 'nbest')

  def __init__(self, index, kind, start_frame, end_frame, first_speech, last_speech, greedy_ids, score):
    self.index, self.kind, self.start_frame, self.end_frame = index, kind, start_frame, end_frame
    self.first_speech, self.last_speech = first_speech, last_speech
    self.greedy_ids, self.score, self.ids, self.logp = greedy_ids, score, greedy_ids, None
    self.spans = self.align_score = self.confidence = self.words = self.nbest = None

  def __repr__(self):
    return 'Utterance({}, {!r}, rows [{}, {}), speech {}..{}, ids={}, logp={}, score={})'.format(
        self.index, self.kind, self.start_frame, self.end_frame, self.first_speech, self.last_speech, self.ids, self.logp, self.score)


class StreamSpotter:
  """Keyword spotting of a `StreamingRecognizer` (st_ctc_spot_stream_step; the rule: include/speecht_hip.h,
  tests/spot_stream_oracle.py).  ``keywords``: the words and phrases, as texts (`spotting.keyword_ids`: letters, apostrophe, space).
  A stretch of frames read as a keyword is a candidate when its score per frame reaches ``threshold`` (<= 0 or -inf; the score of
  `speecht-cli spot`); of overlapping candidates the best stays, and it is reported once a later candidate lies behind it or
  ``hold`` seconds have passed without a better one -- or when the stream finishes (`Hit.flushed`).  The 0.3 s default of ``hold``
  is a guess, not tuned on data.  A step hands back at most ``max_events`` hits per stream; the rest is counted in
  `StepResult.hits_lost`.  One keyword set for all streams."""

  def __init__(self, keywords, threshold=None, hold=0.3, max_events=64):
    from . import spotting
    if isinstance(keywords, str) or not all(isinstance(k, str) for k in keywords):
      raise StreamError('spotting: keywords must be a list of texts')
    self.keywords = [k.lower() for k in keywords]
    if not self.keywords:
      raise StreamError('spotting: no keywords given')
    if len(set(self.keywords)) != len(self.keywords):
      raise StreamError('spotting: a keyword is given twice')
    try:
      self.ids = [spotting.keyword_ids(k) for k in self.keywords]
    except spotting.TranscriptionError as e:
      raise StreamError('spotting: {}'.format(e))
    self.threshold = float(spotting.DEFAULT_THRESHOLD if threshold is None else threshold)
    if np.isnan(self.threshold) or self.threshold > 0:
      raise StreamError('spotting: threshold must be <= 0 or -inf (a score per frame), got {!r}'.format(threshold))
    self.hold = float(hold)
    if not (np.isfinite(self.hold) and self.hold > 0):
      raise StreamError('spotting: hold must be a positive number of seconds, got {!r}'.format(hold))
    if not isinstance(max_events, (int, np.integer)) or isinstance(max_events, bool) or max_events < 1:
      raise StreamError('spotting: max_events must be a positive integer, got {!r}'.format(max_events))
    self.max_events = int(max_events)

  def frames(self, total_stride, frame_rate=None):
    """``hold`` in output frames of a model whose layers' strides multiply to ``total_stride``, counted as `Endpointing.frames`
    counts: rounded up, at least 1.  ``frame_rate``: feature frames per second (None: the 10 ms hop)."""
    return seconds_to_frames(self.hold, total_stride, frame_rate)

  def plan(self, num_classes, pack=1):
    """-> (the plan of st_ctc_spot_stream_plan as an int32 array, its waves).  Runs on the host."""
    if not 2 <= num_classes <= 32:
      raise StreamError('spotting supports 2..32 classes, the engine has {}'.format(num_classes))
    if max(max(i) for i in self.ids) > num_classes - 2:
      raise StreamError('spotting: a keyword has a character the model\'s {} classes do not hold'.format(num_classes))
    lib = _lib.load()
    ids = np.asarray([i for k in self.ids for i in k], dtype=np.int32)
    offs = np.cumsum([0] + [len(k) for k in self.ids]).astype(np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    size = int(lib.st_ctc_spot_stream_plan_bytes(p(ids), p(offs), len(self.ids), num_classes, pack))
    if not size:
      raise StreamError('spotting: {}'.format(lib.st_last_error().decode()))
    words, waves = np.zeros(size // 4, dtype=np.int32), ctypes.c_int(0)
    call('st_ctc_spot_stream_plan', p(ids), p(offs), len(self.ids), num_classes, pack, p(words), ctypes.byref(waves))
    return words, waves.value


class Hit:
  """A keyword a step has found: ``keyword`` (the text) and its ``index`` in the spotter's list, the stream's logits rows
  ``[start_frame, end_frame)`` (absolute: they count from the stream's start, whatever endpointing cut), ``score`` (<= 0, as
  `speecht-cli spot` reports it) and ``flushed`` -- the stream finished while the hit was still waiting for a better one."""
  __slots__ = ('keyword', 'index', 'start_frame', 'end_frame', 'score', 'flushed')

  def __init__(self, keyword, index, start_frame, end_frame, score, flushed):
    self.keyword, self.index, self.start_frame, self.end_frame = keyword, int(index), int(start_frame), int(end_frame)
    self.score, self.flushed = float(score), bool(flushed)

  @property
  def score_per_frame(self):
    return self.score / (self.end_frame - self.start_frame)

  def __eq__(self, other):
    return isinstance(other, Hit) and all(getattr(self, n) == getattr(other, n) for n in Hit.__slots__)

  def __repr__(self):
    return 'Hit({!r}, {}, rows [{}, {}), score={!r}{})'.format(self.keyword, self.index, self.start_frame, self.end_frame, self.score,
                                                             ', flushed' if self.flushed else '')


def read_hits(keywords, events, counts, max_events):
  """The host's part of a spotting step: ``events`` int32 [S, max_events, 8] and ``counts`` [S] as the device left them ->
  per stream (hits sorted by (end_frame, index), hits lost: the events beyond ``max_events``)."""
  out = []
  for ev, count in zip(events, counts.tolist()):
    if count == 0:                                                # (most streams, most steps)
      out.append(([], 0))
      continue
    kept = ev[:min(count, max_events)]
    score = np.ascontiguousarray(kept[:, 4:6]).view(np.float64).reshape(-1)
    hits = [Hit(keywords[k], k, a, e, sc, kind == 1) for (k, a, e, kind), sc in zip(kept[:, :4].tolist(), score.tolist())]
    out.append((sorted(hits, key=lambda h: (h.end_frame, h.index)), max(count - max_events, 0)))
  return out


class ScriptFollower:
  """Following a known script in the streams of a `StreamingRecognizer` (st_ctc_follow_stream_step; the rule: include/speecht_hip.h,
  tests/follow_oracle.py): a stream opened with ``open(script=...)`` reports after every step where in its script the speaker is
  (`StepResult.follow`) and which words have just been reached (`StepResult.reached`).  The script's alignment lattice is carried
  across steps in tiles, so a script may be long: ``max_labels`` ids per stream (1 .. 28 671; the state of a stream is two columns
  of that many label and blank states in double).  A word counts as reached once the best state has stayed at or behind its first
  character for ``confirm`` seconds (1 .. 16 output frames: the cursor of a Viterbi filter jumps on noise); the 0.06 s default is a
  guess, not tuned on data.  A step hands back at most ``max_events`` reached words per stream, the rest is counted in
  `StepResult.reached_lost`.  ``trace``: every step also returns the best state of each of its rows (``follow[slot]['trace']``).
  ``space_id``: the class that separates words ('auto': 27 with the 29 classes a-z ' space blank, none otherwise; -1: none -- the
  script is one word).  Exact start and end times of the words are `speecht-cli align --segment`'s, on the recording."""

  def __init__(self, max_labels=16384, confirm=0.06, max_events=64, trace=False, space_id='auto'):
    if not isinstance(max_labels, (int, np.integer)) or isinstance(max_labels, bool) or not 1 <= max_labels <= 28671:
      raise StreamError('following: max_labels must lie in 1..28671, got {!r}'.format(max_labels))
    self.max_labels = int(max_labels)
    self.confirm = float(confirm)
    if not (np.isfinite(self.confirm) and self.confirm > 0):
      raise StreamError('following: confirm must be a positive number of seconds, got {!r}'.format(confirm))
    if not isinstance(max_events, (int, np.integer)) or isinstance(max_events, bool) or max_events < 1:
      raise StreamError('following: max_events must be a positive integer, got {!r}'.format(max_events))
    self.max_events, self.trace = int(max_events), bool(trace)
    if space_id != 'auto' and (not isinstance(space_id, (int, np.integer)) or space_id < -1):
      raise StreamError('following: space_id must be \'auto\', -1 or a class index, got {!r}'.format(space_id))
    self.space_id = space_id

  def frames(self, total_stride, frame_rate=None):
    """``confirm`` in output frames, counted as `StreamSpotter.frames` counts ``hold``: rounded up, at least 1; more than 16 is
    refused.  ``frame_rate``: feature frames per second (None: the 10 ms hop)."""
    k = seconds_to_frames(self.confirm, total_stride, frame_rate)
    if k > 16:
      raise StreamError('following: confirm = {} s is {} output frames, at most 16 are kept'.format(self.confirm, k))
    return k

  def space(self, num_classes):
    space = (27 if num_classes == 29 else -1) if self.space_id == 'auto' else int(self.space_id)
    if space >= num_classes - 1:
      raise StreamError('following: space_id {} is no label of a model with {} classes'.format(space, num_classes))
    return space

  def script(self, script, num_classes):
    """A text (`vocabulary.sentence_to_ids` after lower-casing) or a list of ids -> (ids, the first label index of every word,
    the words as texts).  Refuses an empty script, one without a word, one beyond ``max_labels`` and ids the model has no label
    for."""
    from . import vocabulary
    if isinstance(script, str):
      try:
        ids = vocabulary.sentence_to_ids(script)
      except Exception as e:
        raise StreamError('following: the script has a character outside the vocabulary ({})'.format(e))
    else:
      try:
        ids = [int(i) for i in script]
      except (TypeError, ValueError):
        raise StreamError('following: a script is a text or a list of ids, got {!r}'.format(type(script).__name__))
    if not ids:
      raise StreamError('following: the script is empty')
    if len(ids) > self.max_labels:
      raise StreamError('following: the script has {} ids, max_labels = {}'.format(len(ids), self.max_labels))
    if min(ids) < 0 or max(ids) > num_classes - 2:
      raise StreamError('following: the script has an id outside the model\'s labels 0..{}'.format(num_classes - 2))
    space = self.space(num_classes)
    starts = [i for i, l in enumerate(ids) if l != space and (i == 0 or ids[i - 1] == space)]
    if not starts:
      raise StreamError('following: the script has no word')
    ends = [next((j for j in range(a, len(ids)) if ids[j] == space), len(ids)) for a in starts]
    letter = (lambda i: vocabulary.id_to_letter(i)) if num_classes == vocabulary.SIZE + 1 else (lambda i: '<{}>'.format(i))
    return ids, starts, [''.join(letter(i) for i in ids[a:e]) for a, e in zip(starts, ends)]


class WordReached:
  """A word of its script a followed stream has reached: its ``index`` among the script's words, its ``text`` and the output
  ``frame`` (absolute, counted from the stream's start) at which the rule confirmed it."""
  __slots__ = ('index', 'text', 'frame')

  def __init__(self, index, text, frame):
    self.index, self.text, self.frame = int(index), text, int(frame)

  def __eq__(self, other):
    return isinstance(other, WordReached) and (self.index, self.text, self.frame) == (other.index, other.text, other.frame)

  def __repr__(self):
    return 'WordReached({}, {!r}, frame {})'.format(self.index, self.text, self.frame)


def read_follow(records, events, max_events, scripts, slots):
  """The host's part of a following step: ``records`` int32 [S, 16] and ``events`` int32 [S, max_events, 2] as the device left them,
  ``scripts`` per slot (ids, word starts, words) -> {slot: (dict frames / state / label / word / in_blank / fit / end_score /
  complete / status, [WordReached], events lost)} for the ``slots`` asked for.  ``label``: the script's id index the best state
  stands at or has last left (-1 before the first); ``word``: the index of the word that label belongs to or follows (-1 before the
  first word); ``complete``: the end state is the best state."""
  import bisect
  heads = records[:, :4].tolist()                                # (one conversion for all streams: this runs in every step)
  reals = np.ascontiguousarray(records[:, 4:8]).view(np.float64).tolist()
  out = {}
  for s in slots:
    ids, starts, words = scripts[s]
    (frames, c, status, count), (fit, end) = heads[s], reals[s]
    label = (c - 1) >> 1 if c >= 1 else -1
    state = dict(frames=frames, state=c, label=label, word=bisect.bisect_right(starts, label) - 1 if label >= 0 else -1,
                 in_blank=c >= 0 and c % 2 == 0, fit=fit, end_score=end, complete=c >= 2 * len(ids) - 1, status=status)
    reached = [WordReached(j, words[j], t) for j, t in events[s, :min(count, max_events)].tolist()] if count else []
    out[s] = (state, reached, max(count - max_events, 0))
  return out


class StepResult:
  """What one `step` / `finish` produced: ``ids[slot]`` new label ids, ``logits[slot]`` new rows [r, C] (on request),
  ``score[slot]`` the running negative sum of the chosen logits.  With a beam search also ``hyp[slot]``, all ids of the best
  hypothesis so far, ``stable[slot]``, how many of its leading ids are final, and ``logp[slot]``, its log-probability (after
  `finish`: what the whole-utterance search returns); ``ids`` and ``score`` stay the greedy ones.  With endpointing ``finals[slot]``
  lists the `Utterance`s the step closed, in order; ``hyp`` / ``stable`` / ``logp`` / ``score`` and ``open_ids[slot]`` (the greedy ids
  so far) then describe the utterance still open, and ``ids`` stays every new greedy id of the step.  With a spotter ``hits[slot]``
  lists the `Hit`s the step found, sorted by (end_frame, index), and ``hits_lost[slot]`` counts those that did not fit the
  spotter's ``max_events`` (0 as a rule: raise ``max_events`` otherwise).  With ``StreamBeam(nbest=N)`` ``nbest_lost[slot]`` counts the
  finals of the step whose list did not fit the arena (raise ``nbest_words`` otherwise) and, without endpointing, ``nbest[slot]`` is
  None until `finish` fills it with the stream's list (`Utterance.nbest` describes it; ``hyp`` / ``logp`` follow a rescoring).
  With a `ScriptFollower`, for the streams opened with a script: ``follow[slot]`` where the speaker is (`read_follow`),
  ``reached[slot]`` the `WordReached` of the step in order and ``reached_lost[slot]`` those beyond the follower's ``max_events``."""

  def __init__(self):
    self.ids, self.logits, self.score = {}, {}, {}
    self.hyp, self.stable, self.logp = {}, {}, {}
    self.finals, self.open_ids = {}, {}
    self.hits, self.hits_lost = {}, {}
    self.nbest, self.nbest_lost = {}, {}
    self.follow, self.reached, self.reached_lost = {}, {}, {}


class StepLayout:
  """Where a step's results lie in its one buffer of int32 words (``dec_out``), so that they come back with one copy: the named
  segments in order, ``segments[name] = (first word, length, shape)``, and their ``size`` in all -- no torch, no device.
    ids [S][max_new] | counts [S] | scores [S] (float32)
    with endpointing (``n_pieces`` = P; without it P = 1):  | events [S][P][8] | pieces [P][S][4]
    with a beam search (``max_tail``):                      | result [P][S][4] | tail [P][S][max_tail]
    with a spotter (``spot_events``):                       | spot_counts [S] | spot_events [S][spot_events][8]
    with a follower (``follow_events``), from the next even word on (its records hold doubles):
                                     | follow_records [S][16] | follow_events [S][follow_events][2] | follow_trace [``trace_rows``]
    with N-best lists (``lists``), the last word: used, the words the step's lists asked for (the arena is copied only if not 0)
  The options take their device views from it, and resolve once where a pass's read-outs find theirs in the host copy (`views`)."""

  def __init__(self, S, max_new, n_pieces=None, max_tail=None, spot_events=None, follow_events=None, trace_rows=None, lists=False):
    self.segments, self.size = {}, 0
    P = 1 if n_pieces is None else n_pieces
    self._add('ids', S, max_new), self._add('counts', S), self._add('scores', S)
    if n_pieces is not None:
      self._add('events', S, P, 8), self._add('pieces', P, S, 4)
    if max_tail is not None:
      self._add('result', P, S, 4), self._add('tail', P, S, max_tail)
    if spot_events is not None:
      self._add('spot_counts', S), self._add('spot_events', S, spot_events, 8)
    if follow_events is not None:
      self.size += self.size & 1
      self._add('follow_records', S, 16), self._add('follow_events', S, follow_events, 2)
      if trace_rows is not None:
        self._add('follow_trace', trace_rows)
    if lists:
      self._add('used', 1)

  def _add(self, name, *shape):
    length = int(np.prod(shape))
    self.segments[name] = (self.size, length, shape)
    self.size += length

  def views(self, *names):
    """-> f(words): the named segments of ``words`` -- the device buffer or a host copy of it -- each in its shape."""
    cuts = [(slice(first, first + length), shape) for first, length, shape in map(self.segments.get, names)]
    return lambda words: [words[cut].reshape(shape) for cut, shape in cuts]


def read_beam(hyp, stable, row, tail, max_tail, final):
  """One read-out of a streamed beam search: ``hyp`` / ``stable``, the hypothesis the host holds and how many of its leading ids are
  final; ``row`` = {length, stable, log-probability (float32 bits), status} and ``tail``, the labels above ``stable``, as the device left
  them.  -> ``(hyp, stable, logp, head)``, the tail appended above ``head``, the ids that were final (a ``final`` read-out's hypothesis
  is final as a whole) -- or the reason, a text, why the read-out gave up."""
  length, old = int(row[0]), int(stable)
  if row[3] != 0:
    return 'status {}'.format(int(row[3]))
  if length - old > max_tail or length < old:
    return '{} labels are not final yet, max_tail = {}'.format(length - old, max_tail)
  head = hyp[:old]
  return head + tail[:length - old].tolist(), length if final else int(row[1]), row[2:3].view(np.float32)[0], head


def _upload(engine, array, dtype):
  """Host array -> device on the engine's stream (pinned staging from torch's caching host allocator: no wait for the stream's earlier
  kernels, and the block is not reused before the copy has run)."""
  host = torch.from_numpy(array).pin_memory()
  with torch.cuda.stream(engine.stream):
    return host.to(engine.device, non_blocking=True)


# What an option adds to a `StreamingRecognizer`, made only when the option is given: its checks of the engine, its device state and
# segments of the step's buffer, its state per slot, and the hooks the recogniser calls in a fixed order -- ``reset`` a slot at `open`,
# ``seed`` the slots' entries of a fresh `StepResult`, ``launch`` for a pass (-> the kernels enqueued), ``read`` its share of the host copy.
# ``src``: the pass's rows as every decoder takes them (logits, pitch, classes, the (stream, frame) of every row); ``table``: the
# decoders' {first row, rows, limit, fresh} per stream.

class _EndpointPart:
  unfetched = 'endpointing: the utterances the step closes'          # what a step with fetch=False would lose

  def __init__(self, rec, frames):                               # `Endpointing.frames`: (R, L, M, space)
    lib, S, dev = _lib.load(), rec.max_streams, rec.device
    self.engine, self.max_new, self.frames, self.n_pieces = rec.engine, rec.max_new, frames, rec.n_pieces
    self.state = torch.zeros(S * int(lib.st_stream_endpoint_state_bytes()) // 4, dtype=torch.int32, device=dev)
    self.score = torch.zeros(S * int(lib.st_stream_endpoint_score_bytes()) // 4, dtype=torch.float32, device=dev)
    self.events, self.pieces = rec.layout.views('events', 'pieces')(rec.dec_out)
    self.host = rec.layout.views('ids', 'counts', 'events', 'pieces')
    self.open_ids = [[] for _ in range(S)]                       # the greedy ids of every slot's open utterance

  def reset(self, slot):
    self.open_ids[slot] = []

  def seed(self, result, slots):
    for s in slots:
      result.finals[s], result.open_ids[s] = [], list(self.open_ids[s])

  def launch(self, src, table, S, greedy_out):     # in the greedy decoder's place: events, and per utterance a table of its own (pieces)
    ptr = self.engine._ptr
    R, L, M, space = self.frames
    call('st_ctc_greedy_endpoint_stream', *src, table, S, space, R, L, M, self.max_new, ptr(self.state), ptr(self.score), *greedy_out,
         ptr(self.events), ptr(self.pieces), self.n_pieces, self.engine.stream_ptr)

  def read(self, words, named, result):
    """The events close utterances in order, each with the greedy ids up to its ``ids_end``.  -> ({slot: the `Utterance`s the pass
    closed}, the slots whose last event dropped what was open: it held no speech, the pieces of the pass)."""
    ids, counts, events, pieces = self.host(words)
    closed, dropped = {}, set()
    for s in named:
      closed[s], prev, last_kind = [], 0, 0
      for e in (events[s].tolist() if events[s, 0, 0] else ()):   # (most steps close nothing)
        if e[0] == 0:
          break
        self.open_ids[s] += ids[s, prev:e[5]].tolist()
        prev, last_kind = e[5], e[0]
        if e[0] in Endpointing.KINDS:
          closed[s].append(Utterance(e[7], Endpointing.KINDS[e[0]], e[1], e[2], e[3], e[4], self.open_ids[s],
                                     float(np.asarray(e[6], np.int32).view(np.float32))))
        self.open_ids[s] = []
      self.open_ids[s] += ids[s, prev:counts[s]].tolist()
      result.open_ids[s] = list(self.open_ids[s])
      result.finals[s] += closed[s]
      if last_kind == 3:
        dropped.add(s)
    return closed, dropped, pieces


class _BeamPart:
  def __init__(self, rec, endpoint, arena_words):                # the recogniser's `_EndpointPart` or None; `StreamBeam.arena_words`
    beam, lib, S, dev, C = rec.beam, _lib.load(), rec.max_streams, rec.device, rec.num_classes
    if beam.lm is not None and C != 29:
      raise StreamError('a language model needs the 29 classes a-z \' space blank, the engine has {}'.format(C))
    if not 2 <= C <= 32:
      raise StreamError('the beam search supports 2..32 classes, the engine has {}'.format(C))
    self.engine, self.beam, self.S = rec.engine, beam, S
    self.lm_args = lambda: (self.lm_handle, beam.lm_weight, beam.word_count_weight, beam.valid_word_count_weight, beam.oov_score)
    self.max_frames = seconds_to_frames(beam.max_seconds, rec.total_stride, rec.frame_rate)     # output frames a node pool holds
    if endpoint is not None:
      self.max_frames = endpoint.frames[2]                         # no utterance is longer: the pool is never full
    self.lm_handle = beam.lm.device_handle(dev) if beam.lm is not None else None
    from .engine_decode import beam_input_transform
    self.transform = beam_input_transform(beam.input_transform)
    state_bytes = int(lib.st_ctc_beam_stream_state_bytes(beam.beam_width, int(beam.lm is not None)))
    self.bias = ()                                                 # the `_bias` entry points' two last arguments
    if beam.hotwords is not None:
      state_bytes = int(lib.st_ctc_beam_stream_bias_state_bytes(beam.beam_width, int(beam.lm is not None)))
      nxt, gain, fin = self._bias_tables = beam.hotwords.device_tables(dev)
      self._bias_struct = _lib.BiasTables(nxt.data_ptr(), gain.data_ptr(), fin.data_ptr(), beam.hotwords.n_states)
      self.roots = torch.zeros(S, dtype=torch.int32, device=dev)
      self.bias = (ctypes.byref(self._bias_struct), ctypes.c_void_p(self.roots.data_ptr()))
    pool_bytes = int(lib.st_ctc_beam_stream_pool_bytes(self.max_frames, beam.beam_width))
    self.ws_bytes = int(lib.st_ctc_beam_stream_ws(rec.max_rows[-1]))
    self.state = torch.zeros(S * state_bytes // 8, dtype=torch.int64, device=dev)
    self.pool = torch.empty(S * pool_bytes // 8, dtype=torch.int64, device=dev)       # (a chain only holds written nodes)
    self.ws = torch.empty(self.ws_bytes // 4, dtype=torch.float32, device=dev)
    self.host = rec.layout.views('result', 'tail', *(('used',) if arena_words is not None else ()))
    self.result, self.tail, *used = self.host(rec.dec_out)
    self.arena_words = arena_words
    if arena_words is not None:
      # filled with a value no header holds, and again after every pass that wrote: behind the records that fit lies no stale one
      self.arena = torch.full((max(arena_words, 1),), -1, dtype=torch.int32, device=dev)
      self.nbest_args = (self.bias or (None, None)) + (beam.nbest, ctypes.c_void_p(self.arena.data_ptr()), arena_words,
                                                       ctypes.c_void_p(used[0].data_ptr()))
    # per slot: output frames decoded (checked against the pool before a launch), the last hypothesis read (its first `stable` ids are
    # final: the device reports only what follows) and its log-probability, a read-out gave up, the hotword set (the lists' `bias`)
    self.frames, self.stable, self.failed = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64), np.zeros(S, dtype=bool)
    self.hyp, self.logp, self.slot_set = [[] for _ in range(S)], np.zeros(S, dtype=np.float32), np.zeros(S, dtype=np.int64)

  def reset(self, slot, index):                                  # (the hotword set's root goes to the device ahead of the first step)
    if self.beam.hotwords is not None:
      with torch.cuda.stream(self.engine.stream):
        self.roots[slot:slot + 1].fill_(self.beam.hotwords.root(index))
    self.slot_set[slot] = index
    self.frames[slot], self.failed[slot] = 0, False
    self._clear(slot)

  def _clear(self, slot):
    self.hyp[slot], self.stable[slot], self.logp[slot] = [], 0, 0.0

  def seed(self, result, slots):
    for s in slots:
      result.hyp[s], result.stable[s], result.logp[s] = list(self.hyp[s]), int(self.stable[s]), float(self.logp[s])
      if self.arena_words is not None:
        result.nbest[s], result.nbest_lost[s] = None, 0

  def plan(self, named, fresh, fin, limit, first, count):
    """Before a pass by table: the rows the searches will take (none at or past a finishing stream's limit) against the pools' capacity.
    -> (the rows taken, the streams the read-out reports on)."""
    taken = np.where(fin, np.clip(limit - first, 0, count), count)
    full = self.frames[named] + taken > self.max_frames
    if full.any():
      k = int(np.flatnonzero(full)[0])
      raise StreamError('stream {}: {} output frames would pass the beam search\'s node pool ({} frames, max_seconds = {})'.format(
          int(named[k]), int(self.frames[named[k]] + taken[k]), self.max_frames, self.beam.max_seconds))
    return taken, (count > 0) | fin | fresh

  def launch_table(self, src, table, n_rows, fetch):             # the read-out only when fetched: what the device calls final, the host holds
    bm, ptr, sp = self.beam, self.engine._ptr, self.engine.stream_ptr
    biased = '_bias' if self.bias else ''
    call('st_ctc_beam_stream_step' + biased, *src, table, n_rows, self.S, bm.beam_width, self.transform, *self.lm_args(),
         ptr(self.state), ptr(self.pool), self.max_frames, ptr(self.ws), self.ws_bytes, sp, *self.bias)
    if not fetch:
      return 2 if n_rows else 1
    name, extra = 'st_ctc_beam_stream_read' + biased, self.bias
    if self.arena_words is not None:                               # one launch more: the counter's reset
      name, extra = 'st_ctc_beam_stream_read_nbest', self.nbest_args
    call(name, table, self.S, bm.beam_width, *self.lm_args(), ptr(self.state), ptr(self.pool), self.max_frames, ptr(self.tail),
         bm.max_tail, ptr(self.result), sp, *extra)
    return (2 if n_rows else 1) + (2 if self.arena_words is not None else 1)

  def launch_pieces(self, src, pieces, n_pieces, n_rows):        # searches and read-outs piece by piece, no host wait in between
    bm, ptr = self.beam, self.engine._ptr
    name, extra = 'st_ctc_beam_stream_step_pieces' + ('_bias' if self.bias else ''), self.bias
    if self.arena_words is not None:                               # the finals' lists into the arena; one launch more (the counter's reset)
      name, extra = 'st_ctc_beam_stream_step_pieces_nbest', self.nbest_args
    call(name, *src, ptr(pieces), n_pieces, n_rows, self.S, bm.beam_width, self.transform, *self.lm_args(), ptr(self.state),
         ptr(self.pool), self.max_frames, ptr(self.ws), self.ws_bytes, ptr(self.tail), bm.max_tail, ptr(self.result),
         self.engine.stream_ptr, *extra)
    return (1 if self.arena_words is not None else 0) + (1 if n_rows else 0) + 2 * n_pieces

  def read(self, words, named, fin, result, read=None, closed=None, dropped=(), pieces=None):
    """The read-outs of a pass.  By table: one per stream that ``read`` names, a final where the stream finishes.  Endpointed (``closed`` /
    ``dropped`` / ``pieces``: `_EndpointPart.read`): the pieces in order -- one marked reset starts from an empty hypothesis, every read-out
    appends above the stable length the one before stored, one with a limit is a final, the next of ``closed[slot]``, and the search starts
    again.  -> None, or the first `StreamError` of a search that gave up (the other streams' results are complete)."""
    res, tail, *used = self.host(words)
    arena, used = None, int(used[0][0]) if used else None
    if used:                                                      # a pass with finals: one more copy (and wait) for what their lists wrote;
      with torch.cuda.stream(self.engine.stream):                 # the fill value goes back in its place behind the copy
        written = self.arena[:min(max(used, 0), self.arena_words)]
        arena = written.cpu().numpy()
        written.fill_(-1)
    failed, listed, unwanted = None, [], set()
    for k, s in enumerate(named):
      if closed is None:                                          # {piece, final, reset} of every read-out the device made for the stream
        walk = [(0, fin[k], False)] if read[k] else []
      else:
        walk = [(p, limit >= 0, reset) for p, (_, rows, limit, reset) in enumerate(pieces[:, s].tolist()) if rows or limit >= 0 or reset]
      at = 0
      for p, final, reset in walk:
        if reset:
          self._clear(s)
        got = read_beam(self.hyp[s], self.stable[s], res[p, s], tail[p, s], self.beam.max_tail, final)
        if isinstance(got, str):
          self.failed[s] = True
          failed = failed or StreamError('stream {}: the beam search gave up ({})'.format(s, got))
          unwanted.update((q, s) for q in range(p, len(res)))     # (the device wrote this final's record, and its later ones', all the same)
          break
        (self.hyp[s], self.stable[s], self.logp[s], head), utt = got, None
        if final and closed is not None:                          # the whole-utterance search on the utterance's rows alone
          utt, at = closed[s][at], at + 1
          utt.ids, utt.logp = self.hyp[s], float(self.logp[s])
          self._clear(s)
        if final and used is not None:
          listed.append((s, (p, s), head, utt))
      if fin[k] and s in dropped:                                 # what was open at the end held no speech: dropped like any discard
        self._clear(s)
      result.hyp[s], result.stable[s], result.logp[s] = list(self.hyp[s]), int(self.stable[s]), float(self.logp[s])
    if listed:                                                    # (lists, then rescoring: the words are those of the ids that are reported)
      self.final_lists(arena, used, listed, result, unwanted)
    return failed

  def final_lists(self, arena, used, listed, result, unwanted=()):
    """The N-best lists of the finals a pass closed, ``listed`` = [(slot, (piece, slot), the ids the host holds below the record's stable
    length, the `Utterance` or -- `finish` without endpointing -- None)]: the arena's records become lists (`nbest.read_arena`), get
    their parts together (`nbest.components`) and with ``rescore`` are re-ranked together, the reported ids and log-probability becoming
    the first hypothesis's.  A record that did not fit counts in ``result.nbest_lost``.  ``unwanted``: the keys of finishing read-outs the
    host gave up on; their records are stepped over, so that one stream's failure never costs the others their lists."""
    from . import nbest as nb
    bm = self.beam
    found, _ = nb.read_arena(arena if arena is not None else np.zeros(0, np.int32), used if arena is not None else 0,
                             {key: head for _, key, head, _ in listed}, skip=unwanted)
    have = [f for f in listed if f[1] in found]
    for slot, key, _, _ in listed:
      if key not in found:
        result.nbest_lost[slot] += 1
    if not have:
      return
    hot = None
    if bm.hotwords is not None:                                   # set 0 is the empty set: no bias
      hot = [bm.hotwords.tables(int(self.slot_set[slot])) if self.slot_set[slot] else None for slot, _, _, _ in have]
    lists = nb.components(self.engine, bm.lm, [found[key] for _, key, _, _ in have],
                          (bm.lm_weight, bm.word_count_weight, bm.valid_word_count_weight), hotwords=hot)
    if bm.rescore is not None:
      r = bm.rescore
      lists = nb.rescored(lists, self.engine, r['language_model'], r['lm_weight'], r['word_count_weight'], r['valid_word_count_weight'])
    for (slot, _, _, utt), hyps in zip(have, lists):
      if utt is not None:
        utt.nbest = hyps
        if bm.rescore is not None:
          utt.ids, utt.logp = list(hyps[0]['ids']), float(hyps[0]['log_prob'])
      else:
        result.nbest[slot] = hyps
        if bm.rescore is not None:
          self.hyp[slot], self.logp[slot] = list(hyps[0]['ids']), hyps[0]['log_prob']
          self.stable[slot] = len(self.hyp[slot])
          result.hyp[slot], result.stable[slot], result.logp[slot] = list(self.hyp[slot]), int(self.stable[slot]), float(hyps[0]['log_prob'])


class _WordsPart:
  def __init__(self, rec, endpoint):                             # the recogniser's `_EndpointPart` (`FinalWords.check` made sure of it)
    self.engine, self.want, self.S, self.C = rec.engine, rec.words, rec.max_streams, rec.num_classes
    self.space = endpoint.frames[3]
    from . import alignment                                        # frames_to_seconds(f, rate) = f * total_stride / frames per second
    self.rate = 2.0 * alignment.HOP_LENGTH * (100.0 if rec.frame_rate is None else rec.frame_rate) / rec.total_stride
    # the ring of logits rows per stream the finals' lattices read (st_stream_keep_rows: M + the rows of a pass)
    self.ring_cap = int(_lib.load().st_stream_keep_rows(endpoint.frames[2], rec.max_new))
    self.ring = torch.zeros(self.S * self.ring_cap * 32, dtype=torch.float32, device=rec.device)

  def launch(self, src, n_rows):                                 # the pass's rows into the ring
    call('st_stream_keep_f32', *src, n_rows, self.S, self.engine._ptr(self.ring), self.ring_cap, self.engine.stream_ptr)
    return 1

  def read(self, finals):
    """The word times and confidences of the finals a pass closed, ``[(slot, Utterance)]``: one table (`final_jobs`), one upload, the ring
    lattices for all of them, one copy back -- the pass's second wait (the next pass's keep overwrites the ring).  -> the kernels enqueued."""
    from . import alignment
    from .engine_decode import MAX_ALIGN_LABELS
    want, launches = self.want, 0
    for _, u in finals:
      if len(u.ids) == 0:
        u.words = []
        if want.timestamps:
          u.spans = np.zeros((0, 2), dtype=np.int32)
    space = self.space if want.confidence else None
    tab = final_jobs([(s, u.start_frame, u.end_frame, u.ids) for s, u in finals], space, MAX_ALIGN_LABELS)
    J = len(tab['index'])
    if not J:
      return 0
    lib = _lib.load()
    eng, S, C = self.engine, self.S, self.C
    N, W, T, max_len = int(tab['offsets'][-1]), len(tab['word_spans']), tab['max_rows'], tab['max_len']
    parts = [tab['jobs'].reshape(-1), tab['ids'], tab['offsets'], tab['word_spans'].reshape(-1), np.zeros(1, np.int32)]
    offs = np.cumsum([0] + [p.size for p in parts])
    table = _upload(eng, np.concatenate(parts), torch.int32)
    tptr = lambda i: ctypes.c_void_p(table.data_ptr() + 4 * int(offs[i]))
    ptr, sp = eng._ptr, eng.stream_ptr
    with torch.cuda.stream(eng.stream):
      # the outputs in one buffer, one copy back: log_conf [W] | log_prob [J] (doubles) | spans [N][2] | score [J] | status [J] | status [J]
      out = torch.zeros(2 * (W + J) + 2 * N + 3 * J, dtype=torch.int32, device=eng.device)
      at = lambda first: ctypes.c_void_p(out.data_ptr() + 4 * first)
      o_spans = 2 * (W + J)
      o_score, o_st_align, o_st_conf = o_spans + 2 * N, o_spans + 2 * N + J, o_spans + 2 * N + 2 * J
      if want.timestamps:
        need = int(lib.st_ctc_align_ws(J, T, max_len))
        ws = torch.empty(need // 4 + 16, dtype=torch.int32, device=eng.device)
        call('st_ctc_align_ring_f32', ptr(self.ring), S, self.ring_cap, C, tptr(0), J, T, tptr(1), tptr(2), max_len, at(o_spans), None,
             at(o_score), at(o_st_align), ptr(ws), ws.numel() * 4, sp)
        launches += 3
      if want.confidence:
        need = int(lib.st_ctc_word_conf_ws(J, T, max_len, J + W))
        ws2 = torch.empty(need // 4 + 16, dtype=torch.int32, device=eng.device)
        call('st_ctc_word_conf_ring_f32', ptr(self.ring), S, self.ring_cap, C, tptr(0), J, T, tptr(1), tptr(2), max_len, space, tptr(3), W,
             at(2 * W), at(0), at(o_st_conf), ptr(ws2), ws2.numel() * 4, sp)
        launches += 3
      host = out.cpu().numpy()                                     # the second wait of a pass that closed something
    log_conf, log_prob = host[:2 * W].view(np.float64), host[2 * W:o_spans].view(np.float64)
    spans, score = host[o_spans:o_score].reshape(N, 2), host[o_score:o_st_align].view(np.float32)
    first_word = np.concatenate([[0], np.cumsum(tab['words'])]).astype(np.int64)
    for j, i in enumerate(tab['index']):
      u = finals[i][1]
      if host[o_st_align + j] != 0 or host[o_st_conf + j] != 0:     # the ids do not fit the rows: nothing, as offline
        continue
      probs = None
      if want.timestamps:
        u.spans = spans[tab['offsets'][j]:tab['offsets'][j + 1]].copy()
        u.align_score = float(score[j])
      if want.confidence:
        probs = np.exp(log_conf[first_word[j]:first_word[j + 1]]).tolist()
        u.confidence = dict(log_prob=float(log_prob[j]), words=probs)
      if want.timestamps:
        u.words = alignment.timed_words(u.ids, u.spans + u.start_frame, self.rate, confidence=probs)
      else:
        u.words = alignment.confident_words(u.ids, probs)
    return launches


class _SpotPart:
  unfetched = 'a spotter: the hits the step finds'

  def __init__(self, rec):
    spot, lib, S, dev = rec.spot, _lib.load(), rec.max_streams, rec.device
    self.engine, self.spot, self.S = rec.engine, spot, S
    self.hold = spot.frames(rec.total_stride, rec.frame_rate)
    self.plan, self.waves = spot.plan(rec.num_classes)             # the host copy: the step reads its header
    self.plan_dev = torch.from_numpy(self.plan).to(dev)
    self.plan_ptr = self.plan.ctypes.data_as(ctypes.c_void_p)
    call('st_ctc_spot_stream_plan_bind', self.plan_ptr, ctypes.c_void_p(self.plan_dev.data_ptr()))
    self.state = torch.zeros(S * int(lib.st_ctc_spot_stream_state_bytes(self.plan_ptr)) // 8, dtype=torch.int64, device=dev)
    self.host = rec.layout.views('spot_events', 'spot_counts')
    self.events, self.counts = self.host(rec.dec_out)

  def seed(self, result, slots):
    for s in slots:
      result.hits[s], result.hits_lost[s] = [], 0

  def launch(self, src, table, n_rows):                          # by the greedy decoder's table: endpointing does not reset spotting
    ptr = self.engine._ptr
    call('st_ctc_spot_stream_step', *src, table, n_rows, self.S, self.plan_ptr, self.spot.threshold, self.hold, ptr(self.state),
         ptr(self.events), self.spot.max_events, ptr(self.counts), self.engine.stream_ptr)
    return 2                                                       # the memset of the counts and the lattices

  def read(self, words, named, result):
    found = read_hits(self.spot.keywords, *self.host(words), self.spot.max_events)
    for s in named:
      result.hits[s] += found[s][0]
      result.hits_lost[s] += found[s][1]


class _FollowPart:
  unfetched = 'a follower: the words the step reaches'

  def __init__(self, rec):
    fw, lib, S, dev = rec.follow, _lib.load(), rec.max_streams, rec.device
    if not 2 <= rec.num_classes <= 32:
      raise StreamError('following supports 2..32 classes, the engine has {}'.format(rec.num_classes))
    fw.space(rec.num_classes)
    self.engine, self.follow, self.S, self.max_rows = rec.engine, fw, S, rec.max_rows[-1]
    self.confirm = fw.frames(rec.total_stride, rec.frame_rate)
    self.state = torch.zeros(S * int(lib.st_ctc_follow_stream_state_bytes(fw.max_labels)) // 8, dtype=torch.float64, device=dev)
    self.ws_bytes = int(lib.st_ctc_follow_stream_ws(self.max_rows, fw.max_labels, S))
    self.ws = torch.empty(self.ws_bytes // 8 + 1, dtype=torch.float64, device=dev)
    self.host = rec.layout.views('follow_records', 'follow_events', *(('follow_trace',) if fw.trace else ()))
    self.records, self.events, self.trace = (self.host(rec.dec_out) + [None])[:3]
    self.scripts = [None] * S                                      # per slot (ids, word starts, words) or None
    self.frames = np.zeros(S, dtype=np.int64)                      # rows each followed stream has consumed (for the trace)
    self._set_scripts()

  def _set_scripts(self):
    """The scripts of all slots as CSR arrays on the device: [script offsets S + 1 | word offsets S + 1 | ids | word starts], one
    upload on the engine's stream (a slot without a script has an empty one and sits out)."""
    S = self.S
    ids = [sc[0] if sc else [] for sc in self.scripts]
    starts = [sc[1] if sc else [] for sc in self.scripts]
    offs, woffs = np.cumsum([0] + [len(i) for i in ids]), np.cumsum([0] + [len(w) for w in starts])
    flat = np.concatenate([offs, woffs, [i for l in ids for i in l], [0], [w for l in starts for w in l], [0]]).astype(np.int32)
    self.table = _upload(self.engine, flat, torch.int32)
    base = self.table.data_ptr()
    at = [0, S + 1, 2 * (S + 1), 2 * (S + 1) + int(offs[-1]) + 1]
    self.script_ptrs = tuple(ctypes.c_void_p(base + 4 * a) for a in (at[2], at[0], at[3], at[1]))   # ids, offsets, starts, offsets

  def reset(self, slot, parsed):                                 # `ScriptFollower.script` of the slot's script; None: not followed
    if parsed is not None or self.scripts[slot] is not None:
      self.scripts[slot], self.frames[slot] = parsed, 0
      self._set_scripts()

  def seed(self, result, slots):
    for s in slots:
      if self.scripts[s] is not None:
        result.follow[s], result.reached[s], result.reached_lost[s] = None, [], 0

  def launch(self, src, table, n_rows, longest):                 # as the spotter; ``longest``: the most rows of a stream in the pass
    fw, ptr = self.follow, self.engine._ptr
    call('st_ctc_follow_stream_step', *src, table, n_rows, self.max_rows, longest, self.S, *self.script_ptrs, fw.max_labels,
         self.confirm, ptr(self.state), ptr(self.events), fw.max_events, ptr(self.records),
         ptr(self.trace) if fw.trace else None, ptr(self.ws), self.ws_bytes, self.engine.stream_ptr)
    return (1 if n_rows else 0) + 2 * max(-(-longest // 64), 1)    # the softmax, then tiles and read-out per 64 rows

  def read(self, words, named, row0, result):                    # ``row0``: every named stream's first row in the pass (for the trace)
    fw, (records, events, *trace) = self.follow, self.host(words)
    followed = read_follow(records, events, fw.max_events, self.scripts, [s for s in named if self.scripts[s] is not None])
    for k, s in enumerate(named):
      if s not in followed:
        continue
      state, reached, lost = followed[s]
      if fw.trace:
        took = state['frames'] - int(self.frames[s])               # (rows at or past a finishing stream's limit are not consumed)
        state['trace'] = (result.follow[s]['trace'] if result.follow.get(s) else []) + \
            trace[0][int(row0[k]):int(row0[k]) + took].tolist()
      self.frames[s] = state['frames']
      result.follow[s] = state
      result.reached[s] += reached
      result.reached_lost[s] += lost


class StreamingRecognizer:
  """Owns the per-layer windows, the workspace and the decoder state of up to ``max_streams`` streams on the engine's device.

  ``open()`` -> slot; ``step({slot: features[t, C]})`` advances all named slots in one pass over the layers and returns the new
  ids per slot; ``finish(slot)`` flushes with the right padding; ``close(slot)`` frees the slot."""

  def __init__(self, engine, max_streams, max_chunk_frames=64, beam=None, endpoint=None, spot=None, words=None, frame_rate=None,
               follow=None):
    """``frame_rate``: feature frames per second, the features' sample rate / hop -- what turns the seconds of ``endpoint``, ``spot``,
    ``beam.max_seconds`` and the words' times into frames and back; None: 100, the 10 ms hop of 16 kHz audio.  ``words``: a `FinalWords` (needs ``endpoint``) -- every final then also carries its words' times and / or confidences
    (`Utterance.spans` / ``align_score`` / ``confidence`` / ``words``): one launch more per pass, and in a pass that closes an utterance
    one upload, the lattices' launches and a second wait.  None: nothing changes.  ``spot``: a `StreamSpotter` -- every step then also reports the keywords it has found (`StepResult.hits`), with or without
    a beam search and endpointing, whose results it does not change: one launch more per step (and the memset of its counts).
    ``follow``: a `ScriptFollower` -- the streams opened with ``open(script=...)`` are followed through their scripts
    (`StepResult.follow` / ``reached``), with or without the other options, whose results it does not change: one table upload at
    `open`, and per pass the softmax launch and two launches per 64 rows of the longest stream; its record rides in the step's copy.
    ``beam``: a `StreamBeam` -- every step then also advances a beam search per stream (`StepResult.hyp` / ``stable`` /
    ``logp``); None: greedy decoding only.  ``endpoint``: an `Endpointing` -- the device cuts every stream into utterances
    (`StepResult.finals`) and restarts the decoders after each; a beam search's node pool then holds ``endpoint.max_utterance``
    seconds (``beam.max_seconds`` is ignored) and a stream may run for any length."""
    if max_streams < 1 or max_chunk_frames < 1:
      raise StreamError('max_streams and max_chunk_frames must be positive')
    self.beam, self.endpoint, self.spot, self.words, self.follow = beam, endpoint, spot, words, follow
    if follow is not None and not isinstance(follow, ScriptFollower):
      raise StreamError('follow must be a ScriptFollower, got {!r}'.format(type(follow).__name__))
    self.engine, self.device = engine, engine.device
    self.max_streams, self.max_chunk = int(max_streams), int(max_chunk_frames)
    self.layers = engine.layers
    self.geo = [(l.width, l.stride) for l in self.layers]
    for w, s in self.geo:
      if not pad_left_fixed(w, s):
        raise StreamError('a layer of width {} and stride {} has no length-independent left padding'.format(w, s))
    self.num_classes = engine.num_classes
    self.total_stride = int(np.prod([s for _, s in self.geo]))
    if frame_rate is not None and not (np.isfinite(frame_rate) and frame_rate > 0):
      raise StreamError('frame_rate must be a positive number of frames per second, got {!r}'.format(frame_rate))
    self.frame_rate = None if frame_rate is None else float(frame_rate)
    if words is not None:                                        # (refused before anything is allocated)
      if not isinstance(words, FinalWords):
        raise StreamError('words must be a FinalWords, got {!r}'.format(type(words).__name__))
      words.check(endpoint, self.num_classes, endpoint.frames(self.total_stride, self.num_classes, self.frame_rate)[3] if endpoint is not None else -1)
    arena_words = beam.arena_words(self.max_streams) if beam is not None else None
    L, S = len(self.layers), self.max_streams
    self.in_max = max_new_frames(self.geo, self.max_chunk)
    self.cap = [l.width + self.in_max[i] for i, l in enumerate(self.layers)]            # retained (< width) + new
    self.max_rows = [S * self.in_max[i + 1] for i in range(L)]
    self.max_new = self.in_max[L]
    dev = self.device
    self._endpoint = self._beam = self._spot = self._words = self._follow = None     # the options' parts
    with torch.cuda.stream(engine.stream):
      self.windows = [torch.zeros(S * self.cap[i] * l.cin_pitch, dtype=torch.float32, device=dev) for i, l in enumerate(self.layers)]
      self.logits_pitch = self.layers[-1].cout_pitch
      self.logits = torch.zeros(self.max_rows[-1] * self.logits_pitch, dtype=torch.float32, device=dev)
      lib = _lib.load()
      self.ws_bytes = max(int(lib.st_stream_conv_ws(self.max_rows[i], l.width, l.cin_pitch, l.cout)) for i, l in enumerate(self.layers))
      self.workspace = torch.empty(self.ws_bytes // 4, dtype=torch.float32, device=dev)
      self.dec_state = torch.zeros(S * 4, dtype=torch.int32, device=dev)
      self.dec_score = torch.zeros(S, dtype=torch.float64, device=dev)
      self.n_pieces = 1
      if endpoint is not None:                                     # (the pieces of a pass size the step's buffer)
        ep_frames = endpoint.frames(self.total_stride, self.num_classes, self.frame_rate)
        if not 2 <= self.num_classes <= 64:
          raise StreamError('endpointing supports 2..64 classes, the engine has {}'.format(self.num_classes))
        self.n_pieces = int(lib.st_stream_endpoint_pieces(self.max_new, *ep_frames[:3]))
      # the decoders' outputs in one buffer, so that a step's results come back with one copy
      opt = lambda option, name: getattr(option, name) if option is not None else None
      self.layout = StepLayout(S, self.max_new, n_pieces=self.n_pieces if endpoint is not None else None, max_tail=opt(beam, 'max_tail'),
                               spot_events=opt(spot, 'max_events'), follow_events=opt(follow, 'max_events'),
                               trace_rows=self.max_rows[-1] if opt(follow, 'trace') else None, lists=arena_words is not None)
      self.dec_out = torch.zeros(self.layout.size, dtype=torch.int32, device=dev)
      self._host = self.layout.views('ids', 'counts', 'scores')
      ids, counts, scores = self._host(self.dec_out)
      self._greedy_out = (engine._ptr(ids), self.max_new, engine._ptr(counts), engine._ptr(scores))   # as both greedy kernels take them
      if endpoint is not None:
        self._endpoint = _EndpointPart(self, ep_frames)
      if words is not None:
        self._words = _WordsPart(self, self._endpoint)
        self.ring_cap = self._words.ring_cap
      if spot is not None:
        self._spot = _SpotPart(self)
        self.spot_waves = self._spot.waves
      if follow is not None:
        self._follow = _FollowPart(self)
      if beam is not None:
        self._beam = _BeamPart(self, self._endpoint, arena_words)
        self.max_frames = self._beam.max_frames
      table = np.zeros(L * 2, dtype=np.int64)                                          # {float* windows, int32 cap, int32 c_pitch}
      for i, l in enumerate(self.layers):
        table[2 * i] = self.windows[i].data_ptr()
        table[2 * i + 1] = self.cap[i] | (l.cin_pitch << 32)
      self.layer_table = torch.from_numpy(table).to(dev)
    self._seeders = [p for p in (self._endpoint, self._beam, self._spot, self._follow) if p is not None]
    # the host's counters: per stream and layer the frames received and emitted, per stream the input frames in all
    self._open, self._fresh, self._finished = (np.zeros(S, dtype=bool) for _ in range(3))
    self._n, self._e = np.zeros((S, L), dtype=np.int64), np.zeros((S, L), dtype=np.int64)
    self._total = np.zeros(S, dtype=np.int64)
    self._info = np.zeros((L, S, 4), dtype=np.int32)             # {base, n, base, 0} of every stream between steps
    self.launches = 0            # kernels enqueued by the last pass (products count two: slices + epilogue)

  # -- slots --

  def open(self, hotwords=None, script=None):
    """``script`` (with a `ScriptFollower`): the text, or the ids, the stream is to be followed through (`ScriptFollower.script`);
    None: the stream is not followed.
    -> a free slot.  ``hotwords``: the index of the stream's phrase set in the beam search's `hotwords.HotwordSets` (default: the
    one set when the search was given a single `Hotwords`, else set 0, the empty one); its root is written to the slot's entry of the
    device's roots on the engine's stream, ahead of the slot's first step."""
    sets = self.beam.hotwords if self.beam else None
    if hotwords is not None and sets is None:
      raise StreamError('open(hotwords={!r}): the recognizer has no beam search with hotwords'.format(hotwords))
    if script is not None and self.follow is None:
      raise StreamError('open(script=...): the recognizer has no ScriptFollower')
    parsed = self.follow.script(script, self.num_classes) if script is not None else None
    if sets is not None:
      index = self.beam.default_set if hotwords is None else hotwords
      if not isinstance(index, (int, np.integer)) or isinstance(index, bool) or not 0 <= index < len(sets):
        raise StreamError('open(hotwords={!r}): the sets 0..{} exist'.format(hotwords, len(sets) - 1))
    free = np.flatnonzero(~self._open)
    if not len(free):
      raise StreamError('all {} streams are open'.format(self.max_streams))
    i = int(free[0])
    self._open[i], self._fresh[i], self._finished[i] = True, True, False     # the first step resets the slot's decoder state;
    self._n[i], self._e[i], self._total[i] = 0, 0, 0                           # the windows need no clearing: frames outside
    self._info[:, i] = 0                                                       # [0, n) are never read
    if self._beam is not None:
      self._beam.reset(i, int(index) if sets is not None else 0)
    if self._endpoint is not None:
      self._endpoint.reset(i)
    if self._follow is not None:
      self._follow.reset(i, parsed)
    return i

  def close(self, slot):
    self._slot(slot, allow_finished=True)
    self._open[slot] = False
    self._info[:, slot] = 0

  def _slot(self, slot, allow_finished=False):
    if not isinstance(slot, (int, np.integer)) or not 0 <= slot < self.max_streams or not self._open[slot]:
      raise StreamError('stream {} is not open'.format(slot))
    if self._finished[slot] and not allow_finished:
      raise StreamError('stream {} has been finished: close it and open a new one'.format(slot))
    if self._beam is not None and self._beam.failed[slot] and not allow_finished:
      raise StreamError('stream {}: its beam search has failed: close it and open a new one'.format(slot))

  # -- steps --

  def step(self, feeds, return_logits=False, fetch=True):
    """``feeds``: {slot: float array [t, C]} (t may be 0).  A feed longer than ``max_chunk_frames`` is split into several passes.
    ``fetch=False`` only enqueues (no host wait at all) and returns None: the new ids of such a step are dropped (with endpointing,
    a spotter or a follower it is refused: what they report would be lost)."""
    for part in (self._endpoint, self._spot, self._follow):
      if part is not None and not fetch:
        raise StreamError('fetch=False with {} would be lost'.format(part.unfetched))
    return self._run(feeds, (), return_logits, fetch)

  def finish(self, slot, return_logits=False):
    """Flush ``slot`` with the right padding; returns the rest.  The slot stays allocated until `close`."""
    return self._run({}, (slot,), return_logits, True)

  def finish_many(self, slots, return_logits=False):
    return self._run({}, tuple(slots), return_logits, True)

  def _run(self, feeds, finishing, return_logits, fetch):
    c_in = self.layers[0].cin
    arrays = {}
    for slot, x in feeds.items():
      self._slot(slot)
      x = np.asarray(x, dtype=np.float32) if not isinstance(x, torch.Tensor) else x.detach().to('cpu', torch.float32).numpy()
      if x.ndim != 2 or x.shape[1] != c_in:
        raise StreamError('stream {}: features must be [frames, {}], got {}'.format(slot, c_in, tuple(x.shape)))
      arrays[int(slot)] = np.ascontiguousarray(x)
    for slot in finishing:
      self._slot(slot)
    result = StepResult()
    slots = list(arrays) + [int(s) for s in finishing]
    for slot in slots:
      result.ids[slot], result.score[slot] = [], 0.0
      if return_logits:
        result.logits[slot] = []
    for part in self._seeders:
      part.seed(result, slots)
    longest = max([a.shape[0] for a in arrays.values()] + [0])
    passes = max(-(-longest // self.max_chunk), 1)
    for p in range(passes):
      part = {s: a[p * self.max_chunk:(p + 1) * self.max_chunk] for s, a in arrays.items()}
      self._pass(part, finishing if p == passes - 1 else (), result, return_logits, fetch)
    for hits in result.hits.values():                            # (several passes: a later pass may report an earlier end)
      hits.sort(key=lambda h: (h.end_frame, h.index))
    if return_logits:
      for slot, parts in result.logits.items():
        rows = [t.cpu().numpy() for t in parts]
        result.logits[slot] = np.concatenate(rows) if rows else np.zeros((0, self.num_classes), np.float32)
    return result if fetch else None

  def _pass(self, part, finishing, result, return_logits, fetch):
    eng, L, S = self.engine, len(self.layers), self.max_streams
    named = np.asarray(sorted(set(part) | set(int(s) for s in finishing)), dtype=np.int64)
    # 1. size the step on the host (all named streams at once); whatever is refused is refused here
    new = np.asarray([part[s].shape[0] if s in part else 0 for s in named], dtype=np.int64)
    fin, fresh = np.isin(named, [int(s) for s in finishing]), self._fresh[named]
    first, count, base, n_after, new_base = plan_many(self.geo, self._n[named], self._e[named], new, fin)
    over = (n_after - base > np.asarray(self.cap)) | (count > np.asarray(self.in_max[1:]))
    if over.any():
      k, l = np.argwhere(over)[0]
      raise StreamError('stream {}: layer {} would overrun its window ({} frames, capacity {})'.format(
          int(named[k]), int(l), int(n_after[k, l] - base[k, l]), self.cap[l]))
    limit = np.where(fin, decode_limit(self._total[named] + new), -1)
    by_table = self._beam is not None and self._endpoint is None   # the searches take the greedy decoder's table, not the endpointer's pieces
    taken, read = self._beam.plan(named, fresh, fin, limit, first[:, -1], count[:, -1]) if by_table else (None, None)
    info = self._info.copy()                                     # streams that sit this step out keep their windows
    info[:, named, 0], info[:, named, 1], info[:, named, 2] = base.T, n_after.T, new_base.T

    def table_rows(counts, firsts):                              # (stream, first + j) for j < count, stream by stream
      total = int(counts.sum())
      starts = np.cumsum(counts) - counts
      return np.stack([np.repeat(named, counts), np.repeat(firsts - starts, counts) + np.arange(total)], axis=1).astype(np.int32), starts

    rows = [table_rows(count[:, l], first[:, l])[0] for l in range(L)]
    row0 = np.cumsum(count[:, -1]) - count[:, -1]
    dec = np.zeros((S, 4), dtype=np.int32)
    dec[:, 2] = -1
    dec[named, 0], dec[named, 1], dec[named, 2], dec[named, 3] = row0, count[:, -1], limit, fresh
    feed_rows, _ = table_rows(new, self._n[named, 0] - base[:, 0])
    # 2. one table, one upload
    parts = [info.reshape(-1)] + [r.reshape(-1) for r in rows] + [dec.reshape(-1), feed_rows.reshape(-1)]
    offs = np.cumsum([0] + [p.size for p in parts])
    table = _upload(eng, np.concatenate(parts), torch.int32)
    tptr = lambda i: ctypes.c_void_p(table.data_ptr() + 4 * int(offs[i]))
    info_ptr = lambda l: ctypes.c_void_p(table.data_ptr() + 4 * l * S * 4)
    ptr, sp = eng._ptr, eng.stream_ptr
    self.launches = 0
    # 3. the new frames into the first layer's windows
    if len(feed_rows):
      feat = _upload(eng, np.concatenate([part[s] for s in named.tolist() if s in part and part[s].shape[0]]), torch.float32)
      call('st_stream_feed_f32', ptr(feat), self.layers[0].cin, tptr(L + 2), len(feed_rows), S, ptr(self.windows[0]), self.cap[0],
           self.layers[0].cin_pitch, sp)
      self.launches += 1
    # 4. eleven products with their epilogues
    for l, spec in enumerate(self.layers):
      if not len(rows[l]):
        continue
      pf, pb = eng._slice(eng.params, l)
      lastl = l == L - 1
      out = self.logits if lastl else self.windows[l + 1]
      call('st_stream_conv_f32', ptr(self.windows[l]), self.cap[l], spec.cin_pitch, info_ptr(l), tptr(1 + l), len(rows[l]), S, ptr(pf),
           ptr(pb), spec.width, spec.stride, spec.cout, int(spec.relu), ptr(out), self.max_rows[-1] if lastl else self.cap[l + 1],
           spec.cout_pitch, None if lastl else info_ptr(l + 1), ptr(self.workspace), self.ws_bytes, sp)
      self.launches += 2
    # 5. - 7. the words' ring keeps the new rows, the windows move on, and the decoders take the rows: the endpointer or the greedy
    # decoder, the searches and their read-out, the spotter, the follower
    src, dec_table, n_rows = (ptr(self.logits), self.logits_pitch, self.num_classes, tptr(L)), tptr(L + 1), len(rows[-1])
    if self._words is not None and n_rows:
      self.launches += self._words.launch(src, n_rows)
    call('st_stream_advance', ptr(self.layer_table), L, info_ptr(0), S, sp)
    if self._endpoint is not None:
      self._endpoint.launch(src, dec_table, S, self._greedy_out)
    else:
      call('st_ctc_greedy_stream', *src, dec_table, S, ptr(self.dec_state), ptr(self.dec_score), *self._greedy_out, sp)
    self.launches += 2
    if by_table:
      self.launches += self._beam.launch_table(src, dec_table, n_rows, fetch)
    elif self._beam is not None:
      self.launches += self._beam.launch_pieces(src, self._endpoint.pieces, self.n_pieces, n_rows)
    if self._spot is not None:
      self.launches += self._spot.launch(src, dec_table, n_rows)
    if self._follow is not None:
      self.launches += self._follow.launch(src, dec_table, n_rows, int(count[:, -1].max()) if len(named) else 0)
    # 8. the host's counters follow; nothing above waited
    if by_table:
      self._beam.frames[named] = np.where(fresh, 0, self._beam.frames[named]) + taken
    self._n[named], self._e[named] = n_after, first + count
    self._total[named] += new
    self._fresh[named], self._finished[named] = False, fin
    self._info[:, named, 0], self._info[:, named, 1], self._info[:, named, 2] = new_base.T, n_after.T, new_base.T
    if not fetch:
      return
    # 9. one copy: the step's one wait
    with torch.cuda.stream(eng.stream):
      if return_logits:
        view = self.logits.view(-1, self.logits_pitch)
        for k, s in enumerate(named.tolist()):
          if count[k, -1]:
            result.logits[s].append(view[int(row0[k]):int(row0[k] + count[k, -1]), :self.num_classes].clone())
      words = self.dec_out.cpu().numpy()
    # 10. every option reads its segments of the copy; a search that gave up is reported after the others' results are in
    slots, failed = named.tolist(), None
    if self._follow is not None:
      self._follow.read(words, slots, row0, result)
    if self._spot is not None:
      self._spot.read(words, slots, result)
    ids, counts, score = self._host(words)
    score = score.view(np.float32)
    for s in slots:
      result.ids[s] += ids[s, :counts[s]].tolist()
      result.score[s] = float(score[s])
    if self._endpoint is not None:
      closed, dropped, pieces = self._endpoint.read(words, slots, result)
      if self._beam is not None:
        failed = self._beam.read(words, slots, fin, result, closed=closed, dropped=dropped, pieces=pieces)
      if self._words is not None:
        self.launches += self._words.read([(s, u) for s in slots for u in closed[s]])
    elif self._beam is not None:
      failed = self._beam.read(words, slots, fin, result, read=read)
    if failed is not None:
      failed.result = result                                      # the other streams' results of this step
      raise failed


# ---- resampling live streams (csrc/resample_stream.hip) -------------------------------------------------------------------------

RS_ROW = 16                     # int64 words per row of st_resample_stream_f32's table
RS_STATUS = {1: 'a field is negative or too large', 2: 'the window would overrun', 3: 'samples before the window would be needed',
             4: 'the counts contradict the readiness rule', 5: 'the outputs do not fit', 6: 'a tile\'s span does not fit the LDS'}


class _ResampleSlot:
  __slots__ = ('rate', 'n', 'm', 'base', 'parity', 'finished')

  def __init__(self, rate):
    self.rate, self.n, self.m, self.base, self.parity, self.finished = int(rate), 0, 0, 0, 0, False


class StreamingResampler:
  """Up to ``max_streams`` sample streams, each of its own source rate, resampled to ``model_rate`` as the samples arrive
  (st_resample_stream_f32): the concatenated outputs of a stream are `audio_io.resample_kaiser_best_batch`'s samples of the whole
  signal (librosa's resample + fix_length), bit for bit, however the audio was cut.  An output appears once the samples of its right
  wing are in -- (L + 1) / rate seconds after its time, L = `audio_io.resample_taps` -- and `finish` emits the rest.  The host keeps
  every counter (`audio_io.resample_ready` / ``resample_need`` / ``resample_stream_step``) and checks what the kernel checks before
  it launches.  ``max_source_rate`` sizes the streams' windows (2 L + 2 samples each, twice); ``device='cpu'`` runs the host form
  st_resample_stream_host with the same table (no GPU), whose float64 sums of the last pass are in ``last64``."""

  def __init__(self, model_rate, max_streams=1, max_chunk_samples=16000, device='cuda:0', max_source_rate=48000):
    from . import audio_io
    if max_streams < 1 or max_chunk_samples < 1 or int(model_rate) < 1 or int(max_source_rate) < 1:
      raise StreamError('bad StreamingResampler sizes')
    self.model_rate, self.max_streams, self.max_chunk = int(model_rate), int(max_streams), int(max_chunk_samples)
    self.host = str(device) == 'cpu'
    taps = max(audio_io.resample_taps(int(max_source_rate), self.model_rate), audio_io.resample_taps(1, 2))
    self.cap = 2 * taps + 2
    lib = _lib.load()
    self.state_bytes = int(lib.st_resample_stream_state_bytes(self.max_streams, self.cap))
    self.win = np.ascontiguousarray(audio_io._kaiser_best_filter()[0], dtype=np.float64)
    self.slots = [None] * self.max_streams
    self.launches = 0            # passes enqueued (one kernel each)
    if self.host:
      self.device = None
      self.state = np.zeros(self.state_bytes // 8 + 1, dtype=np.int64)
      self.last64 = {}
    else:
      self.device = torch.device(device)
      self.state = torch.zeros(self.state_bytes // 8 + 1, dtype=torch.int64, device=self.device)
      self.status = torch.zeros(self.max_streams, dtype=torch.int32, device=self.device)
      self.out = torch.zeros(1, dtype=torch.float32, device=self.device)
      self._win = audio_io._device_filter(self.device)
      # the table is read by the host function and copied from there in stream order: a ring of pinned rows, each reused only
      # once the copy that read it is done
      self._tables = [torch.zeros(self.max_streams * RS_ROW, dtype=torch.int64).pin_memory() for _ in range(4)]
      self._table_done = [None] * len(self._tables)
      self._turn = 0

  # -- slots --

  def open(self, rate, slot=None):
    """-> a free slot (``slot``: that one) for a stream of ``rate`` Hz.  Nothing is cleared: a stream's first step reads no state."""
    from . import audio_io
    if not isinstance(rate, (int, np.integer)) or isinstance(rate, bool) or not 0 < rate < 2 ** 31:
      raise StreamError('the source rate must be a positive integer, got {!r}'.format(rate))
    try:
      taps = audio_io.resample_taps(int(rate), self.model_rate)
    except ValueError as e:
      raise StreamError(str(e))
    if 2 * taps + 2 > self.cap:
      raise StreamError('{} -> {} Hz keeps {} samples between steps, the windows hold {} (max_source_rate)'.format(
          rate, self.model_rate, 2 * taps + 2, self.cap))
    if rate != self.model_rate and (int(np.ceil(256.0 * rate / self.model_rate)) + 2 * taps + 2) * 4 > 65536:
      raise StreamError('{} -> {} Hz: a tile\'s source span does not fit the LDS'.format(rate, self.model_rate))
    for i, s in enumerate(self.slots):
      if s is None and slot in (None, i):
        self.slots[i] = _ResampleSlot(rate)
        return i
    raise StreamError('all {} streams are open'.format(self.max_streams) if slot is None else 'stream {} is not free'.format(slot))

  def close(self, slot):
    self._slot(slot, True)
    self.slots[slot] = None

  def _slot(self, slot, allow_finished=False):
    if not isinstance(slot, (int, np.integer)) or not 0 <= slot < self.max_streams or self.slots[slot] is None:
      raise StreamError('stream {} is not open'.format(slot))
    if self.slots[slot].finished and not allow_finished:
      raise StreamError('stream {} has been finished: close it and open a new one'.format(slot))
    return self.slots[slot]

  # -- steps --

  def step(self, feeds):
    """``feeds``: {slot: float samples [n] at the slot's rate} -> {slot: new samples at ``model_rate``} (float32 numpy, may be empty).
    Feeds longer than ``max_chunk_samples`` are cut into passes."""
    return self._run(feeds, ())

  def finish(self, slot):
    """Flush: the outputs up to the fix_length target of everything the slot was fed.  Returns the rest of the slot's samples."""
    self._slot(slot)
    return self._run({}, (slot,))[slot]

  def _arrays(self, feeds, finishing):
    arrays = {}
    for slot, y in feeds.items():
      self._slot(slot)
      y = np.ascontiguousarray(np.asarray(y, dtype=np.float32))
      if y.ndim != 1:
        raise StreamError('stream {}: samples must be a one-dimensional array, got shape {}'.format(slot, tuple(y.shape)))
      arrays[int(slot)] = y
    for slot in finishing:
      self._slot(slot)
    return arrays

  def _run(self, feeds, finishing):
    arrays = self._arrays(feeds, finishing)
    result = {s: [] for s in list(arrays) + [int(s) for s in finishing]}
    sums = {s: [] for s in result}
    longest = max([len(a) for a in arrays.values()] + [0])
    passes = max(-(-longest // self.max_chunk), 1)
    for p in range(passes):
      part = {s: a[p * self.max_chunk:(p + 1) * self.max_chunk] for s, a in arrays.items()}
      out, where = self.step_device(part, finishing if p == passes - 1 else ())
      host = out if self.host else out.cpu().numpy()
      if not self.host:
        self._raise_status(self.status.cpu().numpy())
      for s, (at, count) in where.items():
        if count:
          result[s].append(host[at:at + count].copy())
          if self.host:
            sums[s].append(self._pass64[at:at + count].copy())
    if self.host:
      self.last64 = {s: (np.concatenate(r) if r else np.zeros(0, np.float64)) for s, r in sums.items()}
    return {s: (np.concatenate(r) if r else np.zeros(0, np.float32)) for s, r in result.items()}

  def step_device(self, feeds, finishing=()):
    """One pass without a read-back: ``feeds`` {slot: float samples [n <= max_chunk_samples]} and the slots to finish -> (the float32
    device buffer of the pass's outputs, {slot: (offset, count)}); the buffer is laid out as the ``samples`` argument of
    st_melspec_stream_f32, ready on the current stream and valid until the next pass.  A feed longer than ``max_chunk_samples`` is
    refused before anything is launched."""
    arrays = self._arrays(feeds, finishing)
    table, where, after, total = self.plan({s: len(a) for s, a in arrays.items()}, finishing)
    chunks = [arrays[s] for s in sorted(arrays) if len(arrays[s])]
    samples = np.concatenate(chunks) if chunks else np.zeros(1, np.float32)
    if self.host:
      out, self._pass64 = self._launch_host(table, samples, total)
      self._raise_status(self._host_status)
    else:
      d_samples = torch.from_numpy(samples).pin_memory().to(self.device, non_blocking=True)
      out = self.launch(table, d_samples, total)
    self.commit(after)
    return out, where

  def plan(self, news, finishing=()):
    """The table of one pass, from counts alone: ``news`` {slot: new samples} (their samples concatenated in slot order) and the slots
    to finish -> (table int64 [max_streams, 16], {slot: (offset in the outputs, count)}, the counters to `commit` once the pass is
    launched, total outputs).  Refuses (StreamError) what the kernel would refuse by status; changes nothing."""
    from . import audio_io
    table = np.zeros((self.max_streams, RS_ROW), dtype=np.int64)
    where, after, src, total = {}, {}, 0, 0
    finishing = set(int(x) for x in finishing)
    for s in sorted(set(int(x) for x in news) | finishing):
      st = self._slot(s)
      new, fin = int(news.get(s, 0)), s in finishing
      if new > self.max_chunk:
        raise StreamError('stream {}: {} new samples, a pass takes {} (max_chunk_samples)'.format(s, new, self.max_chunk))
      count, n_orig, valid, target = audio_io.resample_stream_step(st.n, st.m, new, fin, st.rate, self.model_rate)
      n1, m1 = st.n + new, st.m + count
      base1 = n1 if fin else min(audio_io.resample_need(m1, st.rate, self.model_rate), n1)
      if st.n - st.base > self.cap or n1 - base1 > self.cap or base1 < st.base:
        raise StreamError('stream {}: {} samples would overrun the window'.format(s, max(st.n - st.base, n1 - base1)))
      if count and st.m < (valid if fin else m1) and audio_io.resample_need(st.m, st.rate, self.model_rate) < st.base:
        raise StreamError('stream {}: output {} needs samples the window has dropped'.format(s, st.m))
      table[s, :14] = (st.rate, st.base, base1, st.n, src, new, st.m, count, total, int(fin), n_orig, valid, target, st.parity)
      where[s] = (total, count)
      after[s] = (n1, m1, base1, fin)
      src += new
      total += count
    return table, where, after, total

  def commit(self, after):
    """Move the counters of the streams of a launched pass on (``after`` from `plan`)."""
    for s, (n1, m1, base1, fin) in after.items():
      st = self.slots[s]
      st.n, st.m, st.base, st.finished, st.parity = n1, m1, base1, fin, st.parity ^ 1

  def launch(self, table, d_samples, total):
    """Enqueue one pass: ``table`` from `plan` (or made by hand), ``d_samples`` the concatenated new samples on the device -> the
    device buffer of the ``total`` outputs.  ``status`` (device int32 [max_streams]) tells which rows the kernel refused."""
    if total > self.out.numel():
      self.out = torch.zeros(total + total // 2, dtype=torch.float32, device=self.device)
    k = self._turn
    self._turn = (k + 1) % len(self._tables)
    if self._table_done[k] is not None:
      self._table_done[k].synchronize()
    self._tables[k].copy_(torch.from_numpy(np.ascontiguousarray(table, dtype=np.int64).reshape(-1)))
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = torch.cuda.current_stream(self.device)
    call('st_resample_stream_f32', P(d_samples), P(self._tables[k]), self.max_streams, self.model_rate, P(self._win), self._win.numel(),
         P(self.state), self.state_bytes, self.cap, P(self.out), int(total), P(self.status), ctypes.c_void_p(stream.cuda_stream))
    self._table_done[k] = torch.cuda.Event()
    self._table_done[k].record(stream)
    self.launches += 1
    return self.out[:total]

  def _launch_host(self, table, samples, total, out=None):
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    table = np.ascontiguousarray(table, dtype=np.int64)
    samples = np.ascontiguousarray(samples, dtype=np.float32)
    out = np.zeros(max(total, 1), np.float32) if out is None else out
    out64 = np.zeros(len(out), np.float64)
    self._host_status = np.zeros(self.max_streams, np.int32)
    call('st_resample_stream_host', p(samples), p(table), self.max_streams, self.model_rate, p(self.win), len(self.win), p(self.state),
         self.state_bytes, self.cap, p(out), p(out64), len(out), p(self._host_status))
    return out[:total], out64[:total]

  def run_table(self, table, samples, total, fill=0.0):
    """A hand-made table, as it is: -> (outputs [total] float32 numpy, status int32 [max_streams]).  The counters are not touched;
    the output buffer holds ``fill`` wherever the pass wrote nothing.  For tests of the kernel's own checks."""
    samples = np.array(samples, dtype=np.float32)
    if self.host:
      out, _ = self._launch_host(table, samples, total, out=np.full(max(total, 1), fill, np.float32))
      return out.copy(), self._host_status.copy()
    if total > self.out.numel():
      self.out = torch.zeros(total + total // 2, dtype=torch.float32, device=self.device)
    self.out.fill_(fill)
    out = self.launch(table, torch.from_numpy(samples).to(self.device), total)
    return out.cpu().numpy(), self.status.cpu().numpy()

  def _raise_status(self, status):
    bad = [(s, int(c)) for s, c in enumerate(status) if c]
    if bad:
      raise StreamError('the resampler refused ' + ', '.join('stream {}: {}'.format(s, RS_STATUS.get(c, c)) for s, c in bad))


# ---- the mel front end -------------------------------------------------------------------------------------------------------

N_FFT = 512


def frames_ready(n, hop, finished):
  """Frames whose log-mel power can be computed after ``n`` samples.  Frame t needs samples t * hop - 256 ... t * hop + 255 (and
  frame 0, reflected at the start, sample 256).  An open stream counts whole pairs (2p, 2p + 1) only: the kernels transform two
  frames with one FFT, and a fixed pairing keeps a frame's value independent of the chunking (at most one hop of delay)."""
  if finished:
    return 1 + n // hop
  if n <= N_FFT // 2:
    return 0
  ready = (n - N_FFT // 2) // hop + 1
  return ready - ready % 2


def sample_base(f, hop):
  """First absolute sample still needed once ``f`` frames are out."""
  return max(f * hop - N_FFT // 2, 0)


class _FeatSlot:
  __slots__ = ('n', 'f', 'fresh', 'finished', 'chunk')

  def __init__(self, chunk=None):
    self.n, self.f, self.fresh, self.finished, self.chunk = 0, 0, True, False, chunk    # chunk: source samples per pass


class StreamingFeatures:
  """Log-mel features of up to ``max_streams`` sample streams, computed as the samples arrive (st_melspec_stream_f32).

  ``stats=None``: causal normalisation -- the first ``warm`` frames appear together with the reference and the statistics of frame
  ``warm - 1`` (the network waits 99 frames for its first output anyway), every later frame with the running ones; an utterance of at
  most ``warm`` frames gets the whole-utterance features.  ``stats=(ref, mean, std)`` (largest mel power, mean and deviation of the dB
  values): fixed statistics, every utterance gets the features those constants give.  Mel features only.

  ``source_rate`` (here, or per stream in `open`): the streams deliver samples at that rate and the front end brings them to
  ``samplerate`` on the device first (a `StreamingResampler` of its own; its outputs are the mel kernel's input in place, only
  features are read back).  The features are then those of `audio_io.resample_kaiser_best_batch`'s samples of the whole signal fed
  at ``samplerate``, bit for bit and however the audio was cut; they lag (L + 1) / source_rate seconds more.  ``max_chunk_samples``
  stays a count at ``samplerate``.  Without any source rate, calls, tables and launches are what they are without the argument."""

  def __init__(self, samplerate, n_mels, max_streams=1, max_chunk_samples=16000, warm=100, stats=None, hop_length=160, device='cuda:0',
               source_rate=None):
    from .preprocessing import mel_filterbank
    if max_streams < 1 or max_chunk_samples < 1 or warm < 1 or not 0 < n_mels <= 256:
      raise StreamError('bad StreamingFeatures sizes')
    self.device = torch.device(device)
    self.n_mels, self.hop, self.warm, self.max_streams = int(n_mels), int(hop_length), int(warm), int(max_streams)
    self.max_chunk = int(max_chunk_samples)
    self.cap = N_FFT + 2 * self.hop + self.max_chunk + 16
    self.max_new = self.max_chunk // self.hop + 4
    self.max_rows = self.max_streams * self.max_new
    self.out_cap = self.warm + self.max_new
    self.stats = None if stats is None else (float(np.log2(max(stats[0], 1e-10))), float(stats[1]), float(stats[2]))
    lib = _lib.load()
    dev = self.device
    basis = torch.as_tensor(mel_filterbank(float(samplerate), N_FFT, self.n_mels).astype(np.float32)).contiguous().to(dev)
    self.plan = torch.zeros(int(lib.st_melspec_plan_bytes()) // 4, dtype=torch.float32, device=dev)
    self._stream = torch.cuda.current_stream(dev)
    call('st_melspec_plan_f32', self._p(basis), self.n_mels, N_FFT, self._p(self.plan), self.plan.numel() * 4, self._sp)
    self.state_bytes = int(lib.st_melspec_stream_state_bytes(self.max_streams, self.cap, self.n_mels, self.warm))
    self.state = torch.zeros(self.state_bytes // 4 + 2, dtype=torch.float32, device=dev)
    self.ws_bytes = int(lib.st_melspec_stream_ws(self.max_rows, self.n_mels))
    self.workspace = torch.empty(self.ws_bytes // 4, dtype=torch.float32, device=dev)
    self.out = torch.zeros(self.max_streams * self.out_cap * self.n_mels, dtype=torch.float32, device=dev)
    self.slots = [None] * self.max_streams
    self.samplerate, self.source_rate, self.resampler = int(samplerate), source_rate, None
    if source_rate is not None:
      self._source_chunk(source_rate)                            # (refuses a rate the front end cannot serve)
    torch.cuda.current_stream(dev).synchronize()                 # (the basis may be freed once the plan is made)

  @staticmethod
  def _p(t):
    return ctypes.c_void_p(t.data_ptr())

  @property
  def _sp(self):
    return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

  def _source_chunk(self, rate):
    """Source samples of ``rate`` Hz a pass may take so that its outputs, a finish's flush included, fit ``max_chunk_samples``."""
    from . import audio_io
    if not isinstance(rate, (int, np.integer)) or isinstance(rate, bool) or not 0 < rate < 2 ** 31:
      raise StreamError('the source rate must be a positive integer, got {!r}'.format(rate))
    try:
      taps = audio_io.resample_taps(int(rate), self.samplerate)
    except ValueError as e:
      raise StreamError(str(e))
    chunk = int((self.max_chunk - 2) * float(rate) / self.samplerate) - (taps + 2)
    if chunk < 1:
      raise StreamError('max_chunk_samples = {} is too small for a stream of {} Hz'.format(self.max_chunk, rate))
    return chunk

  def open(self, source_rate=None):
    """-> a free slot.  ``source_rate``: the rate of this stream's samples (default: the front end's ``source_rate``; None: they are at
    ``samplerate`` already)."""
    rate = self.source_rate if source_rate is None else source_rate
    if rate is None and self.resampler is None:
      for i, s in enumerate(self.slots):
        if s is None:
          self.slots[i] = _FeatSlot()
          return i
      raise StreamError('all {} streams are open'.format(self.max_streams))
    # once a stream is resampled every stream's samples pass through the resampler (equal rates: a copy, bit for bit), so that the
    # mel kernel reads one buffer
    rate = self.samplerate if rate is None else rate
    chunk = self._source_chunk(rate)
    free = [i for i, s in enumerate(self.slots) if s is None]
    if not free:
      raise StreamError('all {} streams are open'.format(self.max_streams))
    if self.resampler is None:
      resampler = StreamingResampler(self.samplerate, self.max_streams, max_chunk_samples=max(chunk, self.max_chunk), device=self.device,
                                     max_source_rate=max(int(rate), 48000))
      for i, s in enumerate(self.slots):
        if s is not None:
          resampler.open(self.samplerate, slot=i)
          s.chunk = self._source_chunk(self.samplerate)
      self.resampler = resampler
    self.resampler.max_chunk = max(self.resampler.max_chunk, chunk)
    self.resampler.open(int(rate), slot=free[0])
    self.slots[free[0]] = _FeatSlot(chunk)
    return free[0]

  def close(self, slot):
    self._slot(slot, True)
    self.slots[slot] = None
    if self.resampler is not None:
      self.resampler.close(slot)

  def _slot(self, slot, allow_finished=False):
    if not isinstance(slot, (int, np.integer)) or not 0 <= slot < self.max_streams or self.slots[slot] is None:
      raise StreamError('stream {} is not open'.format(slot))
    if self.slots[slot].finished and not allow_finished:
      raise StreamError('stream {} has been finished: close it and open a new one'.format(slot))
    return self.slots[slot]

  def step(self, feeds):
    """``feeds``: {slot: float samples [n]} -> {slot: new features [t, n_mels]} (float32 numpy; t may be 0)."""
    return self._run(feeds, ())

  def finish(self, slot):
    """Flush: the frames up to 1 + n // hop, reflected at the end.  Returns the rest of the slot's features."""
    st = self._slot(slot)
    n = st.n
    if self.resampler is not None:
      from . import audio_io
      rs = self.resampler.slots[slot]
      n = audio_io.resample_lengths(rs.n, rs.rate, self.samplerate)[1]
    if n <= N_FFT // 2:
      raise StreamError('stream {}: {} samples, the reflection at the ends needs more than {}'.format(slot, n, N_FFT // 2))
    return self._run({}, (slot,))[slot]

  def _run(self, feeds, finishing):
    arrays = {}
    for slot, y in feeds.items():
      self._slot(slot)
      y = np.ascontiguousarray(np.asarray(y, dtype=np.float32))
      if y.ndim != 1:
        raise StreamError('stream {}: samples must be a one-dimensional array, got shape {}'.format(slot, tuple(y.shape)))
      arrays[int(slot)] = y
    for slot in finishing:
      self._slot(slot)
    result = {s: [] for s in list(arrays) + [int(s) for s in finishing]}
    if self.resampler is None:
      longest = max([len(a) for a in arrays.values()] + [0])
      passes = max(-(-longest // self.max_chunk), 1)
      for p in range(passes):
        part = {s: a[p * self.max_chunk:(p + 1) * self.max_chunk] for s, a in arrays.items()}
        self._pass(part, finishing if p == passes - 1 else (), result)
    else:                                                        # a pass takes what resamples to at most max_chunk samples
      per = {s: self.slots[s].chunk for s in arrays}
      passes = max([-(-len(a) // per[s]) for s, a in arrays.items()] + [1])
      for p in range(passes):
        part = {s: a[p * per[s]:(p + 1) * per[s]] for s, a in arrays.items()}
        self._pass(part, finishing if p == passes - 1 else (), result)
    return {s: (np.concatenate(r) if r else np.zeros((0, self.n_mels), np.float32)) for s, r in result.items()}

  def _resample(self, part, finishing):
    """The resampler's pass in front of the mel kernel's: -> ({slot: samples at ``samplerate`` this pass}, their device buffer)."""
    rs = self.resampler
    table, where, after, total = rs.plan({s: len(a) for s, a in part.items()}, finishing)
    chunks = [part[s] for s in sorted(part) if len(part[s])]
    source = np.concatenate(chunks) if chunks else np.zeros(1, np.float32)
    d_source = torch.from_numpy(source).pin_memory().to(self.device, non_blocking=True)
    out = rs.launch(table, d_source, total)
    rs.commit(after)
    return {s: count for s, (_, count) in where.items()}, (out if total else rs.out[:1])

  def _pass(self, part, finishing, result):
    S = self.max_streams
    minfo = np.zeros((S, 8), dtype=np.int32)
    feed = np.zeros((S, 4), dtype=np.int32)
    for s, st in enumerate(self.slots):
      if st is not None:
        b = sample_base(st.f, self.hop)
        minfo[s] = (b, st.n, b, 0, 0, 0, st.f, 0)
    pairs, after, rows, src, chunks = [], {}, 0, 0, []
    news, d_samples = (None, None) if self.resampler is None else self._resample(part, finishing)
    for s in sorted(set(part) | set(int(x) for x in finishing)):
      st = self.slots[s]
      new = (len(part[s]) if s in part else 0) if news is None else news.get(s, 0)
      fin = s in finishing
      n = st.n + new
      f_new = max(frames_ready(n, self.hop, fin), st.f)
      m = f_new - st.f
      base = sample_base(st.f, self.hop)
      if n - base > self.cap or m > self.max_new:
        raise StreamError('stream {}: {} samples would overrun the window'.format(s, n - base))
      minfo[s] = (base, n, sample_base(f_new, self.hop), int(fin), rows, m, st.f, int(st.fresh))
      feed[s] = (src, new, st.n - base, 0)
      pairs += [(s, t) for t in range(st.f, f_new, 2)]
      if new and d_samples is None:
        chunks.append(part[s])
      if self.stats is not None:
        count = m
      elif st.f < self.warm:
        count = f_new if (f_new >= self.warm or fin) else 0
      else:
        count = m
      after[s] = (n, f_new, fin, count)
      rows += m
      src += new
    table = np.concatenate([minfo.reshape(-1), feed.reshape(-1), np.asarray(pairs, dtype=np.int32).reshape(-1)]).astype(np.int32)
    d_table = torch.from_numpy(table).pin_memory().to(self.device, non_blocking=True)
    if d_samples is None:
      samples = np.concatenate(chunks) if chunks else np.zeros(1, np.float32)
      d_samples = torch.from_numpy(samples).pin_memory().to(self.device, non_blocking=True)
    fixed = self.stats is not None
    ref, mean, std = self.stats if fixed else (0.0, 0.0, 1.0)
    call('st_melspec_stream_f32', self._p(d_samples), self._p(d_table), len(pairs), S, self._p(self.plan), self.n_mels, self.hop, self.warm,
         self.cap, int(fixed), ref, mean, std, self._p(self.state), self.state_bytes, self._p(self.out), self.out_cap, self.max_rows,
         self._p(self.workspace), self.ws_bytes, self._sp)
    view = self.out.view(S, self.out_cap, self.n_mels)
    for s, (n, f_new, fin, count) in after.items():
      st = self.slots[s]
      st.n, st.f, st.fresh, st.finished = n, f_new, False, fin
      if count:
        result[s].append(view[s, :count].cpu().numpy())


def transcribe_stream(engine, chunks, max_chunk_frames=64, return_logits=False, beam=None, endpoint=None, words=None):
  """One stream: feed the feature chunks ([t, C] each) in order, finish, and return ``(ids, partials)`` -- all label ids and the
  list of (input frames so far, ids so far) after every chunk that produced any -- plus the logits [T', C] on request.
  ``beam`` (a `StreamBeam`): the ids are the beam search's hypothesis -- at the end the whole-utterance search's result -- and a
  partial is (input frames so far, hypothesis so far, how many of its leading ids are final) after every chunk that changed either.
  ``endpoint`` (an `Endpointing`): the first value is the list of the stream's `Utterance`s instead, and the partials describe the
  utterance open at the time; ``words`` (a `FinalWords`): every `Utterance` carries its words' times and / or confidences."""
  rec = StreamingRecognizer(engine, 1, max_chunk_frames, beam=beam, endpoint=endpoint, words=words)
  slot = rec.open()
  ids, partials, rows, frames, finals = [], [], [], 0, []
  for chunk in chunks:
    r = rec.step({slot: chunk}, return_logits=return_logits)
    frames += len(chunk)
    if endpoint is not None:
      finals += r.finals[slot]
    if beam:
      if not partials or (r.hyp[slot], r.stable[slot]) != partials[-1][1:]:
        partials.append((frames, r.hyp[slot], r.stable[slot]))
    elif endpoint is not None:
      if r.ids[slot]:
        partials.append((frames, r.open_ids[slot]))
    elif r.ids[slot]:
      ids += r.ids[slot]
      partials.append((frames, list(ids)))
    if return_logits:
      rows.append(r.logits[slot])
  r = rec.finish(slot, return_logits=return_logits)
  if endpoint is not None:
    ids = finals + r.finals[slot]
  elif beam:
    ids = r.hyp[slot]
    partials.append((frames, ids, r.stable[slot]))
  else:
    ids += r.ids[slot]
    partials.append((frames, list(ids)))
  rec.close(slot)
  if return_logits:
    rows.append(r.logits[slot])
    return ids, partials, np.concatenate(rows)
  return ids, partials


# ---- `speecht-cli stream` -----------------------------------------------------------------------------------------------------

def _pcm_chunks(stream, samples_per_chunk):
  """Raw 16-bit little-endian mono PCM from a binary stream -> float32 pieces in [-1, 1) as they arrive."""
  want = 2 * samples_per_chunk
  while True:
    data = stream.read(want)
    if not data:
      return
    data = data[:len(data) // 2 * 2]
    if data:
      yield np.frombuffer(data, dtype='<i2').astype(np.float32) / 32768.0


def stream_audio(engine, pieces, samplerate, n_mels, normalize='running', on_partial=None, max_piece=None, beam=None, endpoint=None,
                 on_final=None, spot=None, on_hit=None, words=None, model_rate=None, on_nbest=None, follow=None, script=None,
                 on_reached=None, on_followed=None):
  """Recognise one stream of sample pieces (float32 arrays at ``samplerate``) -> (ids, seconds of audio).  ``on_partial(seconds,
  ids so far)`` is called after every piece that produced new ids.  ``model_rate``: the rate the model was trained at -- the pieces
  are resampled to it on the device as they arrive (`StreamingFeatures(model_rate, source_rate=samplerate)`), and the seconds of
  ``endpoint``, ``spot``, ``beam`` and the words' times count frames of hop / model_rate seconds; the seconds of the partials stay
  those of the audio.  None: no resampling, the features run at ``samplerate`` with a 10 ms frame assumed, as before.  ``normalize='running'``: causal feature normalisation, live.
  ``normalize='file'``: the whole stream is read first and gets the features of the whole file (the statistics `transcribe` uses),
  which are then fed piece by piece -- not live; it yields what `transcribe --batch-size 1` yields and exists for comparison.
  ``beam`` (a `StreamBeam`): the ids are the beam search's -- at the end the whole-utterance search's result -- and
  ``on_partial(seconds, hypothesis so far, how many of its leading ids are final)`` is called whenever either has changed.
  ``endpoint`` (an `Endpointing`): the stream is cut into utterances; ``on_final(utterance)`` is called as each closes, the partials
  describe the utterance open at the time, and the first value returned is the list of `Utterance`s.
  ``words`` (a `FinalWords`, with ``endpoint``): every `Utterance` carries its words' times and / or confidences.
  ``spot`` (a `StreamSpotter`): ``on_hit(hit)`` is called for every `Hit` as its step finds it; hits a step could not hand back
  (more than ``spot.max_events``) raise a RuntimeWarning.
  ``follow`` (a `ScriptFollower`) with ``script`` (a text or ids): the stream is followed through the script; ``on_reached(word)`` is
  called for every `WordReached` as its step reports it, and ``on_followed(state)`` once at the end with the last
  `StepResult.follow` entry; reached words a step could not hand back raise a RuntimeWarning.
  ``beam`` with ``nbest``: with ``endpoint`` every `Utterance` carries its list; without, ``on_nbest(hypotheses)`` is called once at
  the end with the stream's list (None if it was lost), and the ids returned are its first hypothesis's after any rescoring."""
  hop = 160
  if normalize not in ('running', 'file'):
    raise StreamError('normalize must be running or file, got {!r}'.format(normalize))
  ids, fed, last, finals = [], 0, [([], 0)], []
  feature_rate, source = (samplerate, None) if model_rate is None else (int(model_rate), int(samplerate))
  timing = {} if model_rate is None else dict(frame_rate=float(feature_rate) / hop)
  ratio = float(feature_rate) / float(samplerate)

  def closed(r, slot):
    for u in r.finals[slot]:
      finals.append(u)
      if on_final:
        on_final(u)
    if r.finals[slot]:
      last[0] = ([], 0)

  def found(r, slot):
    if follow is not None and slot in r.reached:
      for w in r.reached[slot]:
        if on_reached:
          on_reached(w)
      if r.reached_lost[slot]:
        import warnings
        warnings.warn('following: {} reached words of one step were lost (max_events = {})'.format(r.reached_lost[slot], follow.max_events),
                      RuntimeWarning)
    if spot is None:
      return
    for h in r.hits[slot]:
      if on_hit:
        on_hit(h)
    if r.hits_lost[slot]:
      import warnings
      warnings.warn('keyword spotting: {} hits of one step were lost (max_events = {})'.format(r.hits_lost[slot], spot.max_events),
                    RuntimeWarning)

  def feed(rec, slot, feats, seconds):
    r = rec.step({slot: feats})
    found(r, slot)
    if endpoint is not None:
      closed(r, slot)
    if beam:
      if (r.hyp[slot], r.stable[slot]) != last[0]:
        last[0] = (r.hyp[slot], r.stable[slot])
        if on_partial:
          on_partial(seconds, list(r.hyp[slot]), r.stable[slot])
    elif endpoint is not None:
      if r.ids[slot] and r.open_ids[slot] and on_partial:
        on_partial(seconds, list(r.open_ids[slot]))
    elif r.ids[slot]:
      ids.extend(r.ids[slot])
      if on_partial:
        on_partial(seconds, list(ids))

  if normalize == 'file':
    pieces = [np.asarray(p, np.float32) for p in pieces]
    y = np.concatenate(pieces) if pieces else np.zeros(0, np.float32)
    if len(y) <= N_FFT // 2:
      raise StreamError('too short: {} samples (the features need more than {})'.format(len(y), N_FFT // 2))
    if source is None:
      front = StreamingFeatures(samplerate, n_mels, 1, max_chunk_samples=16000, warm=1 + len(y) // hop, device=engine.device)
      slot = front.open()
      front.step({slot: y})
      feats = front.finish(slot)
      total = len(y)
    else:                                                        # the whole signal through the streaming resampler, piece by piece
      from . import audio_io
      total = audio_io.resample_lengths(len(y), source, feature_rate)[1]
      if total <= N_FFT // 2:
        raise StreamError('too short: {} samples at {} Hz (the features need more than {})'.format(total, feature_rate, N_FFT // 2))
      front = StreamingFeatures(feature_rate, n_mels, 1, max_chunk_samples=16000, warm=1 + total // hop, device=engine.device,
                                source_rate=source)
      slot = front.open()
      feats = [front.step({slot: p})[slot] for p in pieces]
      feats = np.concatenate(feats + [front.finish(slot)])
    per = max(int(max(len(p) for p in pieces) * ratio) // hop, 1)
    rec = StreamingRecognizer(engine, 1, max_chunk_frames=max(per, 8), beam=beam, endpoint=endpoint, spot=spot, words=words, follow=follow,
                              **timing)
    rslot = rec.open(script=script)
    for at in range(0, len(feats), per):
      feed(rec, rslot, feats[at:at + per], min((at + per) * hop, total) / float(feature_rate))
    fed = len(y)
  else:
    max_piece = int(max_piece or 16000)
    if source is not None:                                       # a piece's outputs and a finish's flush in one pass
      max_piece = int(max_piece * ratio) + 512
    front = StreamingFeatures(feature_rate, n_mels, 1, max_chunk_samples=max_piece, device=engine.device, source_rate=source)
    slot = front.open()
    rec = StreamingRecognizer(engine, 1, max_chunk_frames=max(max_piece // hop + 4, 8), beam=beam, endpoint=endpoint, spot=spot, words=words,
                              follow=follow, **timing)
    rslot = rec.open(script=script)
    for p in pieces:
      p = np.asarray(p, np.float32)
      fed += len(p)
      feed(rec, rslot, front.step({slot: p})[slot], fed / float(samplerate))
    if source is None and fed <= N_FFT // 2:
      raise StreamError('too short: {} samples (the features need more than {})'.format(fed, N_FFT // 2))
    feed(rec, rslot, front.finish(slot), fed / float(samplerate))
  r = rec.finish(rslot)
  found(r, rslot)
  if on_followed and r.follow.get(rslot) is not None:
    on_followed(r.follow[rslot])
  if endpoint is not None:
    closed(r, rslot)
    return finals, fed / float(samplerate)
  if beam:
    if on_nbest and rslot in r.nbest:
      on_nbest(r.nbest[rslot])
    return r.hyp[rslot], fed / float(samplerate)
  ids.extend(r.ids[rslot])
  return ids, fed / float(samplerate)


def endpoint_of(flags):
  """The `Endpointing` the flags of `speecht-cli stream` ask for (None without --endpoint)."""
  if not getattr(flags, 'endpoint', False):
    return None
  return Endpointing(silence=flags.endpoint_silence, lead=flags.endpoint_lead, max_utterance=flags.max_utterance)


def words_of(flags):
  """The `FinalWords` the flags of `speecht-cli stream` ask for (None without --timestamps / --confidence)."""
  stamps, conf = bool(getattr(flags, 'timestamps', False)), bool(getattr(flags, 'confidence', False))
  return FinalWords(timestamps=stamps, confidence=conf) if stamps or conf else None


def final_word_lines(path, utterance):
  """The lines `speecht-cli stream` prints behind a final's line, one per word, in the format of `transcribe --timestamps`:
  path<TAB>start<TAB>end<TAB>word, and <TAB>confidence when the words carry one (start and end are `-` without times)."""
  out = []
  for w in utterance.words or []:
    times = '{:.3f}\t{:.3f}'.format(w['start'], w['end']) if 'start' in w else '-\t-'
    tail = '\t{:.4f}'.format(w['confidence']) if 'confidence' in w else ''
    out.append('{}\t{}\t{}{}'.format(path, times, w['word'], tail))
  return out


def lists_of(flags):
  """The N-best options of `StreamBeam` the flags of `speecht-cli stream` ask for ({} without --nbest): ``nbest`` and, with
  --rescore-language-model, ``rescore`` with the weights `transcribe` gives it (--rescore-lm-weight, else --lm-weight; the word-count
  weights of the first pass).  Refuses (StreamError) --nbest without a beam search or outside 1..the beam width, and the rescoring
  flags without what they apply to; loads nothing."""
  nbest, path = getattr(flags, 'nbest', None), getattr(flags, 'rescore_language_model', None)
  if nbest is None:
    if path is not None or hasattr(flags, 'rescore_lm_weight'):
      raise StreamError('--rescore-language-model and --rescore-lm-weight apply with --nbest only')
    return {}
  if hasattr(flags, 'rescore_lm_weight') and path is None:
    raise StreamError('--rescore-lm-weight applies with --rescore-language-model only')
  model = getattr(flags, 'language_model', None)
  biased = getattr(flags, 'hotwords', None) is not None or bool(getattr(flags, 'hotword', None))
  if not (model or getattr(flags, 'beam_width', 0) or biased):
    raise StreamError('--nbest needs a beam search (--beam-width, --language-model or hotwords)')
  beam = getattr(flags, 'beam_width', 0) or (100 if model else 16)
  if not 1 <= nbest <= beam:
    raise StreamError('--nbest must lie in 1..the beam width ({}), got {}'.format(beam, nbest))
  out = dict(nbest=int(nbest))
  if path is not None:
    out['rescore'] = dict(language_model=path, lm_weight=getattr(flags, 'rescore_lm_weight', flags.lm_weight),
                          word_count_weight=flags.word_count_weight, valid_word_count_weight=flags.valid_word_count_weight)
  return out


def nbest_lines(path, hyps):
  """The lines `speecht-cli stream --nbest` prints for a list, in the format of `transcribe --nbest`:
  path<TAB>rank<TAB>log_prob<TAB>text for ranks 1..n (none for a list that was lost)."""
  from . import vocabulary
  return ['{}\t{}\t{:.4f}\t{}'.format(path, rank, h['log_prob'], vocabulary.ids_to_sentence(h['ids']))
          for rank, h in enumerate(hyps or [], 1)]


def spotter_of(flags):
  """The `StreamSpotter` the flags of `speecht-cli stream` ask for (None without --keywords / --keyword): the keywords of the file,
  then those given one by one, duplicates dropped in order."""
  if getattr(flags, 'keywords', None) is None and not getattr(flags, 'keyword', None):
    return None
  from . import spotting
  keywords = spotting.read_keywords(flags.keywords) if getattr(flags, 'keywords', None) else []
  for k in getattr(flags, 'keyword', None) or []:
    if k.lower() not in keywords:
      keywords.append(k.lower())
  return StreamSpotter(keywords, threshold=getattr(flags, 'spot_threshold', None), hold=getattr(flags, 'spot_hold', 0.3))


def follower_of(flags):
  """The `ScriptFollower` and the script the flags of `speecht-cli stream` ask for ((None, None) without --script / --script-text):
  the text of the file with its line ends and runs of blanks as single spaces, or the text given."""
  path, text = getattr(flags, 'script', None), getattr(flags, 'script_text', None)
  if path is None and text is None:
    return None, None
  if path is not None and text is not None:
    raise StreamError('--script and --script-text exclude each other')
  if path is not None:
    with open(path) as f:
      text = f.read()
  text = ' '.join(text.split())
  follower = ScriptFollower(max_labels=max(len(text), 1) if len(text) <= 28671 else 28671, confirm=getattr(flags, 'follow_confirm', 0.06))
  follower.script(text, 29)                                      # (refused here, before a model is built)
  return follower, text


def reached_line(path, word, total_stride, hop, model_rate):
  """The line `speecht-cli stream` prints per reached word: path<TAB>reached<TAB>index<TAB>word<TAB>time, the time being
  frame * total_stride * hop / model_rate seconds."""
  return '{}\treached\t{}\t{}\t{:.3f}'.format(path, word.index, word.text, word.frame * total_stride * hop / float(model_rate))


def followed_line(path, state):
  """The line `speecht-cli stream` prints at the end for a followed stream: path<TAB>followed<TAB>fit per frame<TAB>complete|open."""
  per_frame = state['fit'] / state['frames'] if state['frames'] else float('nan')
  return '{}\tfollowed\t{:.4f}\t{}'.format(path, per_frame, 'complete' if state['complete'] else 'open')


def hit_line(hit, rate, duration=None):
  """The line `speecht-cli stream` prints per hit: start<TAB>end<TAB>keyword<TAB>score<TAB>score_per_frame (seconds, nominal)."""
  from . import alignment
  sec = lambda f: alignment.frames_to_seconds(f, rate, alignment.HOP_LENGTH, duration)
  return '{:.3f}\t{:.3f}\t{}\t{:.4f}\t{:.4f}'.format(sec(hit.start_frame), sec(hit.end_frame), hit.keyword, hit.score, hit.score_per_frame)


def run_cli(flags):
  """`speecht-cli stream PATH|-`: one line "seconds<TAB>transcript so far" per step that produced text, then the final transcript
  as `transcribe` prints it ("path<TAB>transcript").  With --language-model or --beam-width (the flags of `transcribe`, with their
  meaning there) or hotwords (--hotwords / --hotword / --hotword-weight, as `transcribe` takes them: the beam search biased towards
  the phrases) the transcripts are the beam search's and a partial line is "seconds<TAB>hypothesis so far<TAB>number of its
  leading characters that are final".  With --endpoint the stream is cut into utterances: the partial lines describe the utterance that
  is open, every final prints "utt<TAB>index<TAB>start<TAB>end<TAB>transcript" (seconds, from the first to behind the last row with
  speech) -- with --nbest followed by a line per hypothesis (`nbest_lines`, re-ranked with --rescore-language-model, the final's transcript then being the first one's), with --timestamps / --confidence followed by a line per word (`final_word_lines`) --, and the closing line joins the finals' transcripts with spaces.  With --keywords / --keyword every hit prints
  "start<TAB>end<TAB>keyword<TAB>score<TAB>score_per_frame" (`hit_line`) as soon as its step has found it, between the other lines;
  hits a step could not hand back are a warning on stderr.  With --script / --script-text the stream is followed through the given
  text: every word prints "path<TAB>reached<TAB>index<TAB>word<TAB>time" (`reached_line`) as it is reached, and behind the closing
  line comes "path<TAB>followed<TAB>fit per frame<TAB>complete|open" (`followed_line`).  Creates no train / data / log directory."""
  import contextlib
  import sys
  from . import transcription, vocabulary
  from .speech_input import SingleInputLoader
  from .speech_model import Session, create_default_model
  if flags.feature_type != 'power':
    print('stream: mel features only (MFCC deltas need a look-ahead of their own)', file=sys.stderr)
    return 2
  input_size = transcription.FEATURE_WIDTH['power']
  with contextlib.redirect_stdout(sys.stderr):          # stdout carries the transcripts only
    model = create_default_model(flags, input_size, SingleInputLoader(input_size))
  try:
    beam, endpoint, on_final = None, endpoint_of(flags), None
    spot = spotter_of(flags)
    words = words_of(flags)
    follower, script = follower_of(flags)
    from . import hotwords
    hot = hotwords.from_flags(flags)
    # (hotwords need a beam search: as in `transcribe`, beam 16 unless --beam-width or --language-model says otherwise)
    if getattr(flags, 'language_model', None) or getattr(flags, 'beam_width', 0) or hot is not None:
      from .language_model import LanguageModel
      lm = LanguageModel.load(flags.language_model) if getattr(flags, 'language_model', None) else None
      # a stream's length is not known when it starts: an hour of node pool unless the file says less
      beam = dict(beam_width=flags.beam_width or None, lm=lm, lm_weight=flags.lm_weight, word_count_weight=flags.word_count_weight,
                  valid_word_count_weight=flags.valid_word_count_weight, input_transform=flags.beam_input or 'default', max_seconds=3600.0,
                  hotwords=hot, **lists_of(flags))
    if flags.path == '-':
      rate = int(flags.sample_rate)
      per = max(int(rate * flags.chunk_ms / 1000.0), 1)
      pieces = _pcm_chunks(sys.stdin.buffer, per)
    else:
      samples, rate = transcription.load_native(flags.path)
      per = max(int(rate * flags.chunk_ms / 1000.0), 1)
      pieces = [samples[at:at + per] for at in range(0, len(samples), per)]
    with Session(flags.device) as sess:
      with contextlib.redirect_stdout(sys.stderr):
        model.restore(sess, flags.run_train_dir)
      extra, closing = {}, []
      model_rate = getattr(flags, 'model_rate', 'native')
      model_rate = None if model_rate == 'native' else int(model_rate)
      if model_rate is not None:
        extra['model_rate'] = model_rate
      if spot is not None:
        extra.update(spot=spot, on_hit=lambda h: print(hit_line(h, model_rate or rate), flush=True))
      if follower is not None:
        stride = int(np.prod([l.stride for l in model.engine.layers]))
        extra.update(follow=follower, script=script,
                     on_reached=lambda w: print(reached_line(flags.path, w, stride, 160, model_rate or rate), flush=True),
                     on_followed=lambda st: closing.append(followed_line(flags.path, st)))
      if endpoint is not None:
        frame_s = 0.01 * int(np.prod([l.stride for l in model.engine.layers]))
        if model_rate is not None:                               # the features' own frame: hop / rate
          frame_s = 160.0 / model_rate * int(np.prod([l.stride for l in model.engine.layers]))
        on_final = lambda u: print('\n'.join(['utt\t{}\t{:.2f}\t{:.2f}\t{}'.format(u.index, u.first_speech * frame_s,
                                                                                 (u.last_speech + 1) * frame_s,
                                                                                 vocabulary.ids_to_sentence(u.ids))] +
                                             nbest_lines(flags.path, u.nbest) + final_word_lines(flags.path, u)), flush=True)
        extra.update(endpoint=endpoint, on_final=on_final, words=words)
      if beam:
        if beam.get('nbest') and endpoint is None:                # the stream's list, behind the closing line
          extra['on_nbest'] = lambda hyps: closing.extend(nbest_lines(flags.path, hyps))
        if flags.path != '-':
          beam['max_seconds'] = len(samples) / float(rate) + 1.0
        partial = lambda seconds, ids, stable: print('{:.2f}\t{}\t{}'.format(seconds, vocabulary.ids_to_sentence(ids), stable), flush=True)
        ids, _ = stream_audio(model.engine, pieces, rate, input_size, flags.normalize, partial, max_piece=per, beam=StreamBeam(**beam), **extra)
      else:
        partial = lambda seconds, ids: print('{:.2f}\t{}'.format(seconds, vocabulary.ids_to_sentence(ids)), flush=True)
        ids, _ = stream_audio(model.engine, pieces, rate, input_size, flags.normalize, partial, max_piece=per, **extra)
  except (StreamError, transcription.TranscriptionError, ValueError, OSError) as e:
    print('stream: {}'.format(e), file=sys.stderr)
    return 1
  if endpoint is not None:
    print('\n'.join(['{}\t{}'.format(flags.path, ' '.join(vocabulary.ids_to_sentence(u.ids) for u in ids))] + closing), flush=True)
    return 0
  print('\n'.join(['{}\t{}'.format(flags.path, vocabulary.ids_to_sentence(ids))] + closing), flush=True)
  return 0
