"""Batch inference with length bucketing (BASELINE config 3: conv stack + CTC greedy decode on
variable-length utterances).

The reference pads every batch to its longest member and masks nothing (speech_input.py:37-45,
SURVEY F7), so the ~73 output frames before an utterance's end depend on the padded length of the
batch it happens to be in -- unless ``mask_padding`` (``--mask-padding``) is set: then every utterance's rows past
its own length are zeroed after every layer, and it gets the logits it would get alone.  Bucketing by length keeps
padding -- and therefore wasted convolution work -- small; without the mask, results for an utterance equal what the
reference would produce for the SAME batch composition (that is what the tests check), not for an arbitrary one.
"""
import queue
import threading

import numpy as np

from . import vocabulary


def make_buckets(lengths, batch_size):
  """Indices sorted by length, cut into consecutive batches: returns a list of index lists."""
  order = np.argsort(np.asarray(lengths), kind='stable')
  return [order[i:i + batch_size].tolist() for i in range(0, len(order), batch_size)]


def padding_overhead(lengths, buckets):
  """Fraction of padded frames that are padding, for reporting."""
  lengths = np.asarray(lengths)
  padded = sum(len(b) * int(lengths[b].max()) for b in buckets)
  return 1.0 - float(lengths.sum()) / padded


def _plan(features, batch_size, bucket):
  lengths = [f.shape[0] for f in features]
  buckets = make_buckets(lengths, batch_size) if bucket else [
      list(range(i, min(i + batch_size, len(features)))) for i in range(0, len(features), batch_size)]
  return lengths, buckets


# Whether `transcribe` overlaps host staging / read-back with the GPU by default.  Decided by measurement
# (scripts/bench_inference.py, profiles/r3_inference_config3_*.json: 2 048 utterances, windows >= 0.5 s, median of 5).
DEFAULT_PIPELINE = True
# Decoder streams of the pipelined beam search: a search (one wavefront per utterance) takes a little longer than the forward
# pass of the next batch, so two consecutive batches are searched side by side on the decoder's compute units
# (scripts/bench_decode.py, profiles/r4_decode_config5.json).
BEAM_DECODERS = 2


def transcribe(engine, features, batch_size=64, bucket=True, pipeline=None, beam_width=None, language_model=None, lm_options=None,
               timestamps=False, mask_padding=False, confidence=False, nbest=None, rescore=None, hotwords=None):
  """features: list of [T_i, input_size] arrays.  Returns (list of id lists, list of strings) in the
  input order, decoded greedily (speech_model.py:113-115) batch by batch -- or, with ``beam_width``, by the LM-free prefix
  beam search (the reference's beam search needs its KenLM fork, speech_model.py:101-111; configs[4] asks for beam 16).

  pipeline=True (default: ``DEFAULT_PIPELINE``) overlaps the three stages of consecutive batches: a stager thread pads batch k+1
  into pinned host memory and copies it to the device on its own stream while the GPU runs batch k, and the
  transcripts of batch k are read back (pinned, asynchronous) after batch k+1 has been enqueued.  Same
  launches on the same data as the serial loop, hence identical ids.  With ``beam_width`` the search of batch k runs on a
  decoder stream -- on compute units of its own, `engine.decoder_streams` -- under the forward passes of batches k+1 and
  k+2: one wavefront per utterance searches a little longer than the rest of the chip convolves (configs[4]: 3.9 against
  3.6 ms), so two searches are in flight.

  ``language_model`` (a `language_model.LanguageModel` or a path to an ARPA model): the LM-scored beam search instead, the
  reference's decoder (beam 100 unless ``beam_width`` says otherwise; ``lm_options``: keyword arguments of
  ``engine.lm_beam_search_decode`` -- input_transform, lm_weight, word_count_weight, valid_word_count_weight, oov_score).

  ``timestamps=True``: a third element, one [L, 2] int32 array per utterance -- the first output frame and one past the last
  output frame of every decoded id on the best CTC path of those ids (``engine.align``; `alignment.word_spans` and
  `alignment.frames_to_seconds` turn them into word times).  Whichever decoder ran, its ids are aligned against the logits of
  their batch before the next batch overwrites them, so the batches run one after the other (the serial loop: same launches
  on the same data, hence the same ids as without timestamps).  An utterance that decodes to more than
  ``engine_decode.MAX_ALIGN_LABELS`` ids gets None.  With ``timestamps=False`` nothing changes.

  ``confidence=True``: a further element (after the spans when ``timestamps`` is also set), per utterance
  {'log_prob': ln P(ids) under the CTC distribution, 'words': [confidence of each word of the decoded text]} -- the exact CTC
  word posterior of ``engine.word_confidence``: the probability that the stretch between the word's neighbouring spaces reads
  that word, given the other words.  It is computed after decoding, on the same logits, whichever decoder ran (the serial
  loop, as with timestamps: the ids are those of a run without it); None for a hypothesis of more than MAX_ALIGN_LABELS ids.

  ``mask_padding=True``: the forward pass masks the padding of every batch (``engine.forward(mask_padding=True)``): an utterance
  gets the logits -- to the rounding of two summation orders -- and hence the ids and spans it gets with ``batch_size=1``,
  whatever batch it is in.  Off by default: the launch sequence is then exactly the unmasked one.

  ``nbest=N`` (with ``beam_width`` or ``language_model``; N <= the beam): a last element, per utterance the list of its up to N best
  hypotheses, best first -- dicts {'ids', 'text', 'log_prob', 'acoustic'} and, when a model was involved, {'lm_log10', 'words',
  'valid_words'} (`nbest.components`).  The N-best search runs on the engine's own stream (the serial loop, as with timestamps); its
  first hypothesis is the top path of the search without ``nbest``.  ``rescore``: a dict {'language_model', 'lm_weight' (default: the
  first pass's), 'word_count_weight', 'valid_word_count_weight' (default: the first pass's)} -- every list is re-ranked under that
  model (`nbest.rescored`: 'log_prob' becomes the new score, the LM parts those of the second model).  ``ids`` / texts -- and with
  them ``timestamps`` and ``confidence`` -- are those of the best hypothesis after any rescoring.

  ``hotwords`` (a `hotwords.Hotwords`, or a list of phrases for one with the default weight): the beam search is biased towards the
  phrases (a contact list, product names).  It needs a beam search: beam 16 if neither ``beam_width`` nor a model is given.  The
  biased searches are the N-best kernels, so the serial loop runs with ``n_best = nbest or 1``; the lists are returned only with
  ``nbest``, and their hypotheses then carry 'bias'.  None changes nothing."""
  want_lists = nbest is not None
  if hotwords is not None:
    from .hotwords import Hotwords
    if not isinstance(hotwords, Hotwords):
      hotwords = Hotwords(hotwords)
    if not beam_width and language_model is None:
      beam_width = 16
    nbest = nbest or 1
  if nbest is not None:
    if not (beam_width or language_model is not None):
      raise ValueError('transcribe: nbest needs a beam search (beam_width or language_model)')
  elif rescore is not None:
    raise ValueError('transcribe: rescore applies to N-best lists (nbest=N)')
  forward = (lambda: engine.forward(mask_padding=True)) if mask_padding else engine.forward
  if not features:
    return ([], []) + (([],) if timestamps else ()) + (([],) if confidence else ()) + (([],) if want_lists else ())
  if pipeline is None:
    pipeline = DEFAULT_PIPELINE
  if timestamps or confidence or nbest is not None:
    pipeline = False
  lm_opts = dict(lm_options or {})
  if language_model is not None:
    from .language_model import LanguageModel
    if not isinstance(language_model, LanguageModel):
      language_model = LanguageModel.load(language_model)
    beam_width = beam_width or 100

  def decode_sync():
    if language_model is not None:
      return engine.lm_beam_search_decode(language_model, beam_width, **lm_opts)[0]
    return engine.beam_search_decode(beam_width)[0] if beam_width else engine.greedy_decode()[0]

  first_pass = (float(lm_opts.get('lm_weight', 0.8)), float(lm_opts.get('word_count_weight', 0.0)),
                float(lm_opts.get('valid_word_count_weight', 2.3)))
  if rescore is not None:
    from .language_model import LanguageModel
    rescore = dict(rescore)
    lm2 = rescore.get('language_model')
    if lm2 is None:
      raise ValueError("transcribe: rescore needs a 'language_model'")
    rescore['language_model'] = lm2 if isinstance(lm2, LanguageModel) else LanguageModel.load(lm2)

  def decode_nbest():
    """The lists of the batch the engine holds, split into their parts and re-ranked if asked, each hypothesis with its text."""
    from . import nbest as nbest_lists
    bias = dict(hotwords=hotwords) if hotwords is not None else {}
    if language_model is not None:
      lists = engine.lm_beam_search_decode_nbest(language_model, nbest, beam_width, **dict(lm_opts, **bias))
    else:
      lists = engine.beam_search_decode_nbest(nbest, beam_width, **bias)
    lists = nbest_lists.components(engine, language_model, lists, first_pass, **bias)
    if rescore is not None:
      shared = first_pass if language_model is not None else (0.0, 0.0, 0.0)
      lists = nbest_lists.rescored(lists, engine, rescore['language_model'], rescore.get('lm_weight', first_pass[0]),
                                   rescore.get('word_count_weight', shared[1]), rescore.get('valid_word_count_weight', shared[2]))
    for hyps in lists:
      for h in hyps:
        h['text'] = vocabulary.ids_to_sentence(h['ids'])
    return lists

  def decode_async(decode_stream):
    if language_model is not None:
      return engine.lm_beam_search_decode_async(language_model, beam_width, decode_stream, **lm_opts)
    return engine.beam_search_decode_async(beam_width, decode_stream) if beam_width else engine.greedy_decode_async()

  lengths, buckets = _plan(features, batch_size, bucket)
  ids_out = [None] * len(features)
  spans_out = [None] * len(features)
  conf_out = [None] * len(features)
  nbest_out = [None] * len(features)
  if not pipeline:
    for idx in buckets:
      max_t = max(lengths[i] for i in idx)
      x = np.zeros((len(idx), max_t, features[0].shape[1]), dtype=np.float32)
      for row, i in enumerate(idx):
        x[row, :lengths[i]] = features[i]
      engine.load_batch(x, [lengths[i] for i in idx])
      forward()
      if nbest is not None:
        lists = decode_nbest()
        ids = [hyps[0]['ids'] for hyps in lists]
        for row, i in enumerate(idx):
          nbest_out[i] = lists[row]
      else:
        ids = decode_sync()
      for row, i in enumerate(idx):
        ids_out[i] = ids[row]
      if timestamps:
        spans = _align_current(engine, ids)[0]
        for row, i in enumerate(idx):
          spans_out[i] = spans[row]
      if confidence:
        conf = _confidence_current(engine, ids)
        for row, i in enumerate(idx):
          conf_out[i] = conf[row]
    texts = [vocabulary.ids_to_sentence(s) for s in ids_out]
    return (ids_out, texts) + ((spans_out,) if timestamps else ()) + ((conf_out,) if confidence else ()) + \
        ((nbest_out,) if want_lists else ())

  def collect(handle, idx):
    res = handle.result()
    for row, ids in enumerate(res[0] if beam_width else res):
      ids_out[idx[row]] = ids

  import contextlib
  import torch
  depth = 1                                      # batches whose transcripts are still on their way when the next is enqueued
  if beam_width:
    from .engine import decoder_streams
    compute_stream, decode_stream = decoder_streams(engine.device, BEAM_DECODERS)
    depth = len(decode_stream)
    torch.cuda.synchronize(engine.device)        # weights / buffers written on other streams are in place
    on_compute = lambda: torch.cuda.stream(compute_stream)
  else:
    on_compute = contextlib.nullcontext
  with _PIPELINE_LOCK:               # the pinned staging ring of a device serves one pipeline at a time
    stager = _Stager(engine.device, features, lengths, buckets)
    stager.start()
    pending = []
    try:
      for idx in buckets:
        staged = stager.get()
        with on_compute():
          engine.load_batch(staged, [lengths[i] for i in idx])
          forward()
          handle = decode_async(decode_stream if beam_width else None)
        pending.append((handle, idx))
        if len(pending) > depth:
          collect(*pending.pop(0))
      for item in pending:
        collect(*item)
    finally:
      stager.close()
      if beam_width:
        torch.cuda.synchronize(engine.device)    # nothing of this call is left on the masked streams
  return ids_out, [vocabulary.ids_to_sentence(s) for s in ids_out]


def _align_current(engine, labels, wildcard_bias=None, fit=False):
  """``engine.align`` on the batch the engine holds, with labels the kernel cannot take (longer than MAX_ALIGN_LABELS) left out:
  their spans are None, their score -inf and their status 1.  With a ``wildcard_bias`` or ``fit``: a fourth element, the fits
  (None for a label left out)."""
  from .engine_decode import MAX_ALIGN_LABELS
  long = [len(l) > MAX_ALIGN_LABELS for l in labels]
  kept = [[] if skip else l for l, skip in zip(labels, long)]
  if wildcard_bias is None and not fit:
    spans, score, status = res = engine.align(kept)
  else:
    spans, score, status, fits = res = engine.align(kept, wildcard_bias=wildcard_bias, fit=fit)
  for row, skip in enumerate(long):
    if skip:
      spans[row], score[row, 0], status[row] = None, -np.inf, 1
      if len(res) > 3:
        fits[row] = None
  return res


def _confidence_current(engine, labels):
  """``engine.word_confidence`` on the batch the engine holds -> per utterance {'log_prob': ln P(ids), 'words': [probability per
  word]}; None for labels the kernel cannot take (longer than MAX_ALIGN_LABELS) or that do not fit their frames."""
  from .engine_decode import MAX_ALIGN_LABELS
  long = [len(l) > MAX_ALIGN_LABELS for l in labels]
  conf, log_prob, status = engine.word_confidence([[] if skip else l for l, skip in zip(labels, long)])
  return [None if skip or status[row] != 0 else dict(log_prob=float(log_prob[row, 0]), words=np.exp(conf[row]).tolist())
          for row, skip in enumerate(long)]


def align(engine, features, labels, batch_size=1, bucket=True, mask_padding=False, confidence=False, wildcard_bias=None, fit=False):
  """Forced alignment of known transcripts: features as for `transcribe`, ``labels`` one id list per utterance
  -> (spans, scores, status) in input order: spans[i] an [L_i, 2] int32 array (first output frame, one past the last output
  frame of each id on the best CTC path), scores[i] = ln p(that path), status[i] != 0 where the transcript does not fit the
  utterance's output frames (its spans are -1; None for a transcript of more than MAX_ALIGN_LABELS ids).

  Batched as `transcribe` batches.  ``batch_size=1`` is the default for the reason `transcription` gives: nothing in the
  network is masked, so the logits near the end of an utterance depend on the padded length of its batch, and with them the
  times of its last words -- unless ``mask_padding`` is set, which masks the padding in the forward pass as in `transcribe`.

  ``confidence=True``: a fourth element, per utterance {'log_prob', 'words'} as `transcribe` returns it -- the confidences of the
  GIVEN transcript's words (None where status != 0): a low one marks a word the audio contradicts.

  ``wildcard_bias`` / ``fit`` (``engine.align``): labels may hold ``engine_decode.WILDCARD`` for audio the transcript leaves out,
  and the LAST element of the tuple is the list of per-label fits (float64 arrays; None for a transcript too long).  Not
  together with ``confidence``: the word-posterior lattices do not know the wildcard."""
  wild = wildcard_bias is not None or bool(fit)
  if wild and confidence:
    raise ValueError('align: word confidences are not available with a wildcard or the fit')
  if len(features) != len(labels):
    raise ValueError('align: {} feature arrays and {} label sequences'.format(len(features), len(labels)))
  n = len(features)
  spans_out, score_out, status_out, conf_out, fit_out = [None] * n, [float('-inf')] * n, [1] * n, [None] * n, [None] * n
  if not features:
    return (spans_out, score_out, status_out) + ((conf_out,) if confidence else ()) + ((fit_out,) if wild else ())
  lengths, buckets = _plan(features, batch_size, bucket)
  for idx in buckets:
    max_t = max(lengths[i] for i in idx)
    x = np.zeros((len(idx), max_t, features[0].shape[1]), dtype=np.float32)
    for row, i in enumerate(idx):
      x[row, :lengths[i]] = features[i]
    engine.load_batch(x, [lengths[i] for i in idx])
    if mask_padding:
      engine.forward(mask_padding=True)
    else:
      engine.forward()
    res = _align_current(engine, [labels[i] for i in idx], wildcard_bias, fit)
    spans, score, status = res[:3]
    for row, i in enumerate(idx):
      spans_out[i], score_out[i], status_out[i] = spans[row], float(score[row, 0]), int(status[row])
      if wild:
        fit_out[i] = res[3][row]
    if confidence:
      conf = _confidence_current(engine, [labels[i] for i in idx])
      for row, i in enumerate(idx):
        conf_out[i] = conf[row]
  return (spans_out, score_out, status_out) + ((conf_out,) if confidence else ()) + ((fit_out,) if wild else ())


def align_long(engine, features, labels, batch_size=1, mask_padding=False, return_logits=False, wildcard_bias=None, fit=False):
  """Forced alignment of ONE recording given as its segments: ``features`` the list of the segments' feature arrays in time
  order, ``labels`` the id list of the whole transcript, of any length up to ``engine_decode.MAX_ALIGN_LONG_LABELS`` -- which part
  of the text belongs to which segment is what the alignment finds.  The segments go through the forward pass in the batches
  `align` forms (``batch_size``, ``mask_padding`` as there), each segment's own output frames are copied, in segment order, into
  one [sum T, C] device tensor, and ``engine.align_long`` aligns the transcript against it
  -> (spans [L, 2] int32 in CONCATENATED output frames, score = ln p(best path), status != 0 where the transcript does not fit
  the frames -- spans is None then --, frames: the output frames of each segment; `alignment.concat_frame_seconds` maps a
  concatenated frame to seconds).  ``return_logits``: a fifth element, the gathered logits (None without frames).
  ``wildcard_bias`` / ``fit`` (``engine.align_long``): labels may hold ``engine_decode.WILDCARD``, and the LAST element of the
  tuple is the per-label fit, a float64 array [L] (None where the transcript does not fit)."""
  import torch
  wild = wildcard_bias is not None or bool(fit)
  lengths, buckets = _plan(features, batch_size, True) if features else ([], [])
  frames = [l // 2 for l in lengths]                               # the segments' output frames (engine.ctc_lens)
  first = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
  total = int(first[-1])
  if total == 0:
    return (None, float('-inf'), 1, frames) + ((None,) if return_logits else ()) + ((None,) if wild else ())
  logits = torch.empty((total, engine.num_classes), dtype=torch.float32, device=engine.device)
  for idx in buckets:
    max_t = max(lengths[i] for i in idx)
    x = np.zeros((len(idx), max_t, features[0].shape[1]), dtype=np.float32)
    for row, i in enumerate(idx):
      x[row, :lengths[i]] = features[i]
    engine.load_batch(x, [lengths[i] for i in idx])
    if mask_padding:
      engine.forward(mask_padding=True)
    else:
      engine.forward()
    with torch.cuda.stream(engine.stream):
      out = engine.shape.X[-1].interior()
      for row, i in enumerate(idx):
        logits[int(first[i]):int(first[i + 1])].copy_(out[row, :frames[i]])
  logits.record_stream(engine.stream)
  if wild:
    spans, score, status, fits = engine.align_long(logits, labels, wildcard_bias=wildcard_bias, fit=fit)
  else:
    spans, score, status = engine.align_long(logits, labels)
  return (spans if status == 0 else None, score, status, frames) + ((logits,) if return_logits else ()) + \
      (((fits if status == 0 else None),) if wild else ())


def spot(engine, features, keywords, batch_size=1, bucket=True, mask_padding=False, trace=False):
  """Keyword spotting: features as for `transcribe`, ``keywords`` a list of id lists (`spotting.keyword_ids`), every keyword
  searched in every utterance (``engine.spot``; semantics: include/speecht_hip.h)
  -> (score [N, K] float64, spans [N, K, 2] int32, status [N, K]) in input order: the best occurrence of keyword k in utterance
  i, its score the log-likelihood ratio against the greedy reading of the same output frames (<= 0; -inf and spans of -1 where
  the keyword does not fit the utterance).  ``trace=True``: two more elements, per utterance a [K, T_i'] float64 and a
  [K, T_i'] int32 array over its own T_i' output frames -- the best score of the occurrences ending at each frame and their
  first frame (`spotting.pick_hits` finds several hits in them).

  Batched as `align` batches, and ``batch_size=1`` is the default for the same reason: nothing in the network is masked, so the
  logits near the end of an utterance depend on the padded length of its batch -- unless ``mask_padding`` is set."""
  n, K = len(features), len(keywords)
  score = np.full((n, K), -np.inf)
  spans = np.full((n, K, 2), -1, dtype=np.int32)
  status = np.ones((n, K), dtype=np.int32)
  trace_score, trace_start = [None] * n, [None] * n
  if features and K:
    lengths, buckets = _plan(features, batch_size, bucket)
    for idx in buckets:
      max_t = max(lengths[i] for i in idx)
      x = np.zeros((len(idx), max_t, features[0].shape[1]), dtype=np.float32)
      for row, i in enumerate(idx):
        x[row, :lengths[i]] = features[i]
      engine.load_batch(x, [lengths[i] for i in idx])
      if mask_padding:
        engine.forward(mask_padding=True)
      else:
        engine.forward()
      res = engine.spot(keywords, trace=trace)
      for row, i in enumerate(idx):
        rows = slice(row * K, (row + 1) * K)
        score[i], spans[i], status[i] = res[0][rows], res[1][rows], res[2][rows]
        if trace:
          frames = lengths[i] // 2                               # the utterance's output frames (engine.ctc_lens)
          trace_score[i], trace_start[i] = res[3][rows, :frames].copy(), res[4][rows, :frames].copy()
  return (score, spans, status) + ((trace_score, trace_start) if trace else ())


_STREAMS = {}      # device -> the stagers' copy stream
_PINNED = {}       # (device, depth) -> ring of pinned staging buffers, grow-only
_PIPELINE_LOCK = threading.Lock()


class _Stager(threading.Thread):
  """Pads batches into a small ring of pinned host buffers and copies them to the device on a private stream,
  at most ``depth`` batches ahead of the consumer."""

  def __init__(self, device, features, lengths, buckets, depth=2):
    super().__init__(daemon=True)
    import torch
    self.torch = torch
    self.device, self.features, self.lengths, self.buckets = device, features, lengths, buckets
    self.queue = queue.Queue(maxsize=depth)
    # one copy stream per device for the life of the process (creating a stream per call costs the short pools)
    self.stream = _STREAMS.get(str(device)) or _STREAMS.setdefault(str(device), torch.cuda.Stream(device))
    # [pinned buffer, event of its last H2D]; the buffers outlive the call (pinning host memory costs
    # milliseconds and synchronises the device) and are sized for the largest batch of the plan up front
    self.ring = _PINNED.setdefault((str(device), depth), [[None, None] for _ in range(depth + 2)])
    width = features[0].shape[1]
    need = max(len(idx) * max(lengths[i] for i in idx) for idx in buckets) * width
    for slot in self.ring:
      if slot[0] is None or slot[0].numel() < need:
        if slot[1] is not None:
          slot[1].synchronize()
        slot[0] = torch.empty(need + need // 4, dtype=torch.float32, pin_memory=True)
    self.stop = threading.Event()

  def run(self):
    torch = self.torch
    from .speech_input import StagedBatch
    try:
      width = self.features[0].shape[1]
      for k, idx in enumerate(self.buckets):
        if self.stop.is_set():
          return
        slot = self.ring[k % len(self.ring)]
        max_t = max(self.lengths[i] for i in idx)
        n = len(idx) * max_t * width
        if slot[1] is not None:
          slot[1].synchronize()                                   # the copy that last read this buffer is done
        host = slot[0][:n].view(len(idx), max_t, width)
        x = host.numpy()
        for row, i in enumerate(idx):
          x[row, :self.lengths[i]] = self.features[i]
          x[row, self.lengths[i]:] = 0.0
        with torch.cuda.stream(self.stream):
          dev = torch.empty((len(idx), max_t, width), dtype=torch.float32, device=self.device)
          dev.copy_(host, non_blocking=True)
          event = torch.cuda.Event()
          event.record(self.stream)
        slot[1] = event
        self._put(StagedBatch(dev, event))
    except BaseException as e:                                    # surfaces in the consumer's get()
      self._put(e)

  def _put(self, item):
    while not self.stop.is_set():
      try:
        self.queue.put(item, timeout=0.1)
        return
      except queue.Full:
        continue

  def get(self):
    item = self.queue.get()
    if isinstance(item, BaseException):
      raise item
    return item

  def close(self):
    self.stop.set()
    self.join(timeout=5.0)
