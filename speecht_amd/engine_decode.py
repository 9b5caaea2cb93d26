"""Decoders of the engine (speech_model.py:101-115): greedy CTC decoding, the LM-free prefix beam search and the prefix beam
search with a word n-gram scorer, synchronous and
with their outputs on the way to pinned host memory (`inference.transcribe` overlaps them with the next batches) -- and `align`,
the forced alignment of given labels against the same logits."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import Tensor3, call


class _PendingDecode:
  """Decoder outputs on their way to pinned host memory (``Wav2LetterEngine.greedy_decode_async``).  The engine
  alternates between two host slots: read a handle before issuing the second decode after it."""

  def __init__(self, slot, batch, t_out):
    self._slot, self._batch, self._t_out = slot, batch, t_out

  def result(self):
    ids_host, lens_host, event = self._slot
    event.synchronize()
    lens = lens_host[:self._batch].numpy()
    ids = ids_host[:self._batch * self._t_out].numpy().reshape(self._batch, self._t_out)
    return [ids[b, :lens[b]].tolist() for b in range(self._batch)]


class _PendingBeamDecode:
  """Prefix-beam-search outputs on their way to pinned host memory (``Wav2LetterEngine.beam_search_decode_async``):
  ``result()`` waits for that batch only and returns (list of id lists, log_prob [B, 1])."""

  def __init__(self, slot, batch, t_out):
    self._slot, self._batch, self._t_out = slot, batch, t_out
    self._generation = slot['generation']

  def result(self):
    s = self._slot
    if s['generation'] != self._generation:
      # the slots form a ring of (decoder streams + 1): this handle's pinned buffers and event now belong to a later batch
      raise RuntimeError('beam-search handle read too late: {} further beam_search_decode_async call(s) re-used its slot; read a '
                         'handle before issuing more than len(decode streams) further calls'.format(s['generation'] - self._generation))
    s['event'].synchronize()
    lens = s['lens_h'][:self._batch].numpy()
    ids = s['ids_h'][:self._batch * self._t_out].numpy().reshape(self._batch, self._t_out)
    return ([ids[b, :lens[b]].tolist() for b in range(self._batch)],
            s['score_h'][:self._batch].numpy().reshape(-1, 1).copy())


# the largest workspace lm_beam_search_decode_candidates gives one call: 16 candidates x 64 utterances x 500 frames at beam 100
# hold 410 MB of node pools, so a generation of that size runs in one call
CANDIDATE_WORKSPACE_BYTES = 1 << 30


MAX_ALIGN_LABELS = 511          # labels per utterance of st_ctc_align_f32 (the 16-states-per-lane lattice of st_ctc_loss_grad_f32)


WILDCARD = -1                   # the wildcard label of `align` / `align_long`: audio the transcript leaves out (id num_classes in the C ABI)
WILDCARD_BIAS = -1.0            # its default price per frame, in nats: a guess, not tuned on data
MAX_WILDCARD_CLASSES = 31       # the wildcard takes the slot after the blank in the lattices' 32-wide rows


def wildcard_ids(name, ids, num_classes, wild):
  """The check every label goes through before a lattice kernel indexes rows with its ids: ids in [0, num_classes - 1), and --
  ``wild`` -- WILDCARD, which becomes the id num_classes, never two of them in a row.  -> int32 array (a copy)."""
  ids = np.array(ids, dtype=np.int32).reshape(-1)
  star = ids == WILDCARD
  if wild and num_classes > MAX_WILDCARD_CLASSES:
    raise ValueError('{}: the wildcard needs num_classes <= {}, not {}'.format(name, MAX_WILDCARD_CLASSES, num_classes))
  if ids.size and (not wild and star.any() or int(ids[~star].min(initial=0)) < 0 or int(ids[~star].max(initial=0)) >= num_classes - 1):
    raise ValueError('{}: label ids must lie in [0, {}) (blank = {}){}'.format(
        name, num_classes - 1, num_classes - 1, ' or be WILDCARD' if wild else ''))
  if (star[1:] & star[:-1]).any():
    raise ValueError('{}: two adjacent wildcards'.format(name))
  ids[star] = num_classes
  return ids


def _wildcard_bias(name, wildcard_bias):
  bias = WILDCARD_BIAS if wildcard_bias is None else float(wildcard_bias)
  if not (np.isfinite(bias) and bias <= 0.0):
    raise ValueError('{}: wildcard_bias must be finite and <= 0, not {}'.format(name, wildcard_bias))
  return bias


MAX_ALIGN_LONG_LABELS = 1048575   # labels of the one sequence of st_ctc_align_long_f32
ALIGN_LONG_FRAME_BLOCK = 64       # frames per launch of its tile kernel (csrc/ctc_align_long.hip)
ALIGN_LONG_STATE_BLOCK = 896      # lattice states one workgroup of it owns (plus a halo of 2 * ALIGN_LONG_FRAME_BLOCK)
ALIGN_LONG_WORKSPACE_BYTES = 16 << 30    # the default `max_workspace_bytes` of `align_long`


MAX_SPOT_LABELS = 511           # ids per keyword of st_ctc_spot_f32 (the same lattice)
SPOT_TRACE_BYTES = 256 << 20    # the largest trace (12 bytes per job and frame) one st_ctc_spot_f32 call of `spot` writes
SPOT_KPLS = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16)    # states per lane the lattice kernels are built for (csrc/ctc_lattice.h)


def spot_lattice_kpl(keyword_len):
  """The states-per-lane dispatch a keyword of that many ids needs (csrc/ctc_lattice.h, lattice_kpl): 64 * kpl >= 2 L + 1."""
  return next(k for k in SPOT_KPLS if 64 * k >= 2 * keyword_len + 1)


class CandidateDecodes:
  """Outputs of ``lm_beam_search_decode_candidates`` for P weight triples on B utterances: ``ids`` [P, B, T] int32, ``lens``
  [P, B] int32 (a prefix longer than T keeps its true length), ``log_prob`` [P, B] float32 -- device tensors of ``stream``, the
  stream the engine decoded on -- and ``host()``: one (list of id lists, log_prob [B, 1]) per candidate, like ``lm_beam_search_decode``."""

  def __init__(self, ids, lens, log_prob, stream):
    self.ids, self.lens, self.log_prob, self.stream = ids, lens, log_prob, stream
    self._host = None

  def __len__(self):
    return self.ids.shape[0]

  def _sync(self):
    self.stream.synchronize()                        # (the copies of the callers run on the current stream, maybe another one)

  def lens_host(self):
    self._sync()
    return self.lens.cpu().numpy()

  def host(self):
    if self._host is None:
      self._sync()
      ids, lens, lp = self.ids.cpu().numpy(), self.lens.cpu().numpy(), self.log_prob.cpu().numpy()
      T = ids.shape[2]
      self._host = [([ids[p, b, :min(lens[p, b], T)].tolist() for b in range(ids.shape[1])], lp[p].reshape(-1, 1).copy())
                    for p in range(ids.shape[0])]
    return self._host


def beam_input_transform(name):
  """The `input_transform` code of st_ctc_beam_search_decode_ex: None / 'logits' -> 0, 'log10_softmax' -> 1 (the reference's
  decoder input, tf.log(tf.nn.softmax(logits) + 1e-8) / log(10), speech_model.py:102)."""
  if name in (None, 'logits', 0):
    return 0
  if name in ('log10_softmax', 1):
    return 1
  raise ValueError("input_transform must be None, 'logits' or 'log10_softmax', got {!r}".format(name))


def merge_repeated_labels(seq):
  """tf.nn.ctc_beam_search_decoder(merge_repeated=True) on an output prefix: consecutive equal labels collapse (TF's LabelSeq walk;
  it also collapses genuine double letters, which is why the reference passes False, speech_model.py:110)."""
  return [v for i, v in enumerate(seq) if i == 0 or v != seq[i - 1]]


class DecodeMixin:
  """The decoding entry points of `Wav2LetterEngine` (they read the logits X[-1] and the decoder outputs of the current ShapeState
  and the lengths the batch was loaded with; their host slots and stream are made in the engine's `__init__`)."""

  def greedy_decode(self, merge_repeated=True):
    """tf.nn.ctc_greedy_decoder (speech_model.py:113-115) -> (list of id lists, neg_sum_logits [B,1])."""
    sh = self.shape
    self._wait_uploads()
    call('st_ctc_greedy_decode', sh.X[-1].ref, self._ptr(self.ctc_lens), int(merge_repeated),
         self._ptr(sh.dec_ids), sh.t_out, self._ptr(sh.dec_lens), self._ptr(sh.dec_score), self.stream_ptr)
    lens = sh.dec_lens.cpu().numpy()
    ids = sh.dec_ids.view(-1, sh.t_out).cpu().numpy()
    return [ids[b, :lens[b]].tolist() for b in range(len(lens))], sh.dec_score.cpu().numpy().reshape(-1, 1)

  def greedy_decode_async(self, merge_repeated=True):
    """``greedy_decode`` without the host synchronisation: launches the decoder and the D2H copies of its
    outputs into pinned host buffers and returns a handle; ``handle.result()`` waits for that batch only.  Lets
    a caller enqueue the next batch's forward before it reads this batch's transcripts (inference.transcribe)."""
    sh = self.shape
    self._wait_uploads()
    call('st_ctc_greedy_decode', sh.X[-1].ref, self._ptr(self.ctc_lens), int(merge_repeated),
         self._ptr(sh.dec_ids), sh.t_out, self._ptr(sh.dec_lens), self._ptr(sh.dec_score), self.stream_ptr)
    B, n = sh.dec_lens.numel(), sh.dec_ids.numel()
    self._dec_turn ^= 1
    slot = self._dec_host[self._dec_turn]
    if slot is None or slot[0].numel() < n or slot[1].numel() < B:
      if slot is not None:
        slot[2].synchronize()                                      # a copy into the old buffers may be in flight
      slot = [torch.empty(max(n, 1), dtype=torch.int32, pin_memory=True),
              torch.empty(max(B, 1), dtype=torch.int32, pin_memory=True), torch.cuda.Event()]
      self._dec_host[self._dec_turn] = slot
    stream = self.stream
    with torch.cuda.stream(stream):
      slot[0][:n].copy_(sh.dec_ids, non_blocking=True)
      slot[1][:B].copy_(sh.dec_lens, non_blocking=True)
      slot[2].record(stream)
    return _PendingDecode(slot, B, sh.t_out)

  def beam_search_decode(self, beam_width=16, input_transform=None, merge_repeated=False):
    """LM-free CTC prefix beam search, top path (stock tf.nn.ctc_beam_search_decoder semantics; the
    reference's own beam search needs its KenLM fork, speech_model.py:101-111)
    -> (list of id lists, log_prob [B,1]).  Beams up to 128 (the reference runs 100).  ``input_transform='log10_softmax'``
    searches on log10(softmax(logits) + 1e-8), the reference's decoder input (speech_model.py:102); ``merge_repeated``
    (reference: False, speech_model.py:110) collapses repeated labels of the returned prefix the way TF's decoder does."""
    lib = _lib.load()
    sh = self.shape
    B = sh.dec_lens.numel()
    need = lib.st_ctc_beam_ws(B, sh.t_out, int(beam_width))
    ws = self._storage.view('beam_ws', need // 4 + 16, torch.int32)[0]
    self._wait_uploads()
    call('st_ctc_beam_search_decode_ex', sh.X[-1].ref, self._ptr(self.ctc_lens), int(beam_width), beam_input_transform(input_transform),
         self._ptr(sh.dec_ids), sh.t_out, self._ptr(sh.dec_lens), self._ptr(sh.dec_score),
         self._ptr(ws), ws.numel() * 4, self.stream_ptr)
    lens = sh.dec_lens.cpu().numpy()
    ids = sh.dec_ids.view(-1, sh.t_out).cpu().numpy()
    out = [ids[b, :lens[b]].tolist() for b in range(len(lens))]
    if merge_repeated:
      out = [merge_repeated_labels(seq) for seq in out]
    return out, sh.dec_score.cpu().numpy().reshape(-1, 1)

  def align(self, labels, return_states=False, *, wildcard_bias=None, fit=False):
    """Forced alignment (st_ctc_align_f32; semantics: include/speecht_hip.h, tests/align_oracle.py): the best CTC path of the
    given id lists, one per utterance of the batch, against the logits of the current shape
    -> (list of [L_b, 2] int32 arrays: first frame and one past the last frame of each label, score [B, 1] = ln p(best path),
    status [B]: != 0 where the label does not fit its utterance's frames -- then score = -inf and the spans are -1).
    ``return_states``: a fourth element, [B, T'] int32, the label index of every frame (-1 blank, -2 beyond the utterance).
    Labels hold ids in [0, num_classes - 1) and at most MAX_ALIGN_LABELS of them.

    ``wildcard_bias`` (a float <= 0) or ``fit=True``: st_ctc_align_wild_f32 instead (tests/wildcard_align_oracle.py).  Labels may
    then hold WILDCARD, a label for audio the transcript leaves out: a state like any other (at least one frame, never two in a
    row) whose emission is the frame's largest ln-softmax value plus the bias -- WILDCARD_BIAS when ``wildcard_bias`` is None,
    a guess that nobody has tuned on data; its span is the left-out stretch.  The tuple gains, as its LAST element, a list of
    float64 arrays: the fit of every label, sum over its frames of ln p(its class) - ln p(the frame's best class): 0 where the
    greedy reading spells the label on all its frames, negative otherwise, bias * frames for a wildcard, NaN where status != 0."""
    wild = wildcard_bias is not None or bool(fit)
    bias = _wildcard_bias('align', wildcard_bias) if wild else None
    lib = _lib.load()
    sh = self.shape
    xl = sh.X[-1]
    B, T = xl.batch, xl.frames
    if len(labels) != B:
      raise ValueError('align: {} label sequences for a batch of {}'.format(len(labels), B))
    lens = [len(l) for l in labels]
    offs = np.zeros(B + 1, dtype=np.int32)
    offs[1:] = np.cumsum(lens)
    N, max_len = int(offs[-1]), int(max(lens + [0]))
    if max_len > MAX_ALIGN_LABELS:
      raise ValueError('align: label of length {} is too long for the alignment kernel (max {})'.format(max_len, MAX_ALIGN_LABELS))
    # the kernel indexes LDS rows with the id: it must never see one outside the classes (`wildcard_ids`)
    if wild:
      ids = np.concatenate([wildcard_ids('align', l, self.num_classes, True) for l in labels] + [np.zeros(1, np.int32)])
    else:
      ids = np.concatenate([np.asarray(l, dtype=np.int32).reshape(-1) for l in labels] + [np.zeros(1, np.int32)])
      if N and (int(ids.min()) < 0 or int(ids.max()) >= self.num_classes - 1):
        raise ValueError('align: label ids must lie in [0, {}) (blank = {})'.format(self.num_classes - 1, self.num_classes - 1))
    need = lib.st_ctc_align_ws(B, T, max_len)
    ws = self._storage.view('align_ws', need // 4 + 16, torch.int32)[0]
    # outputs in one buffer, one copy back: spans [N][2] | states [B][T] | status [B] | score [B] (float bits) | a word to
    # bring the fits to 8 bytes | fit [N] (doubles, the wildcard form only)
    words = 2 * N + B * T + 2 * B
    fit0 = words + (words & 1)
    out = self._storage.view('align_out', fit0 + 2 * N + 2, torch.int32)[0]
    at = lambda first: ctypes.c_void_p(out.data_ptr() + 4 * first)
    d_ids, d_offs = self._upload_i32(ids), self._upload_i32(offs)
    self._wait_uploads()
    if wild:
      call('st_ctc_align_wild_f32', xl.ref, self._ptr(d_ids), self._ptr(d_offs), self._ptr(self.ctc_lens), max_len, bias,
           at(0), at(2 * N), at(2 * N + B * T + B), at(2 * N + B * T), at(fit0), self._ptr(ws), ws.numel() * 4, self.stream_ptr)
      words = fit0 + 2 * N
    else:
      call('st_ctc_align_f32', xl.ref, self._ptr(d_ids), self._ptr(d_offs), self._ptr(self.ctc_lens), max_len,
           at(0), at(2 * N), at(2 * N + B * T + B), at(2 * N + B * T), self._ptr(ws), ws.numel() * 4, self.stream_ptr)
    with torch.cuda.stream(self.stream):
      host = out[:words].cpu().numpy()
    spans = host[:2 * N].reshape(N, 2)
    res = ([spans[offs[b]:offs[b + 1]].copy() for b in range(B)],
           host[2 * N + B * T + B:2 * N + B * T + 2 * B].view(np.float32).reshape(-1, 1).copy(),
           host[2 * N + B * T:2 * N + B * T + B].copy())
    if return_states:
      res = res + (host[2 * N:2 * N + B * T].reshape(B, T).copy(),)
    if wild:
      fits = host[fit0:fit0 + 2 * N].view(np.float64)
      res = res + ([fits[offs[b]:offs[b + 1]].copy() for b in range(B)],)
    return res

  def align_long(self, logits, labels, max_workspace_bytes=ALIGN_LONG_WORKSPACE_BYTES, *, wildcard_bias=None, fit=False):
    """Forced alignment of ONE long sequence (st_ctc_align_long_f32; the semantics of `align`, include/speecht_hip.h): the
    best CTC path of ``labels`` -- up to MAX_ALIGN_LONG_LABELS ids in [0, num_classes - 1) -- against ``logits``, a float32
    device tensor [T, C] or [T, pitch] (C = num_classes <= pitch) such as the concatenated output frames of a recording's
    segments -> (spans [L, 2] int32: first frame and one past the last frame of each label, score: ln p(best path) as a Python
    float, status: != 0 where the label does not fit T frames -- then score = -inf and the spans are -1).

    The lattice runs in tiles of ALIGN_LONG_FRAME_BLOCK frames x ALIGN_LONG_STATE_BLOCK states, one launch per frame block.
    Its back-pointers take T * ceil((2 L + 1) / 896) * 224 bytes (an hour with 54 000 characters: 6.8 GB) in the engine's
    storage; a workspace above ``max_workspace_bytes`` is refused with a ValueError that names its size.

    ``wildcard_bias`` / ``fit``: as in `align` -- st_ctc_align_long_wild_f32, labels may hold WILDCARD, and the tuple gains the
    per-label fit, a float64 array [L], as its last element."""
    wild = wildcard_bias is not None or bool(fit)
    bias = _wildcard_bias('align_long', wildcard_bias) if wild else None
    lib = _lib.load()
    C = self.num_classes
    if not (torch.is_tensor(logits) and logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_cuda):
      raise ValueError('align_long: logits must be a float32 device tensor [T, C]')
    T, pitch = int(logits.shape[0]), int(logits.shape[1])
    if T <= 0 or pitch < C:
      raise ValueError('align_long: logits of shape [{}, {}] for {} classes'.format(T, pitch, C))
    ids = np.asarray(labels, dtype=np.int32).reshape(-1)
    L = int(ids.shape[0])
    if L > MAX_ALIGN_LONG_LABELS:
      raise ValueError('align_long: label of length {} is too long for the alignment kernel (max {})'.format(L, MAX_ALIGN_LONG_LABELS))
    # the kernel indexes LDS rows with the id: it must never see one outside the classes (`wildcard_ids`)
    if wild:
      ids = wildcard_ids('align_long', ids, C, True)
    elif L and (int(ids.min()) < 0 or int(ids.max()) >= C - 1):
      raise ValueError('align_long: label ids must lie in [0, {}) (blank = {})'.format(C - 1, C - 1))
    need = int(lib.st_ctc_align_long_ws(T, L))
    if need > max_workspace_bytes:
      raise ValueError('align_long: {} frames x {} labels need a workspace of {} bytes ({:.1f} GiB), above max_workspace_bytes = {}'.format(
          T, L, need, need / 2.0 ** 30, int(max_workspace_bytes)))
    logits = logits.contiguous()
    ws = self._storage.view('align_long_ws', need // 4 + 16, torch.int32)[0]
    # outputs in one buffer, one copy back: score (a double) | status, a spare word | spans [L][2] | fit [L] (doubles, the
    # wildcard form only)
    out = self._storage.view('align_long_out', 4 + 4 * L + 2, torch.int32)[0]
    at = lambda first: ctypes.c_void_p(out.data_ptr() + 4 * first)
    d_ids = self._upload_i32(np.concatenate([ids, np.zeros(1, np.int32)]))
    self._wait_uploads()
    self.stream.wait_stream(torch.cuda.current_stream(self.device))    # (the caller made ``logits`` on the current stream)
    if wild:
      call('st_ctc_align_long_wild_f32', self._ptr(logits), T, C, pitch, self._ptr(d_ids), L, bias, at(4), at(0), at(2),
           at(4 + 2 * L), self._ptr(ws), ws.numel() * 4, self.stream_ptr)
    else:
      call('st_ctc_align_long_f32', self._ptr(logits), T, C, pitch, self._ptr(d_ids), L, at(4), at(0), at(2), self._ptr(ws),
           ws.numel() * 4, self.stream_ptr)
    with torch.cuda.stream(self.stream):
      host = out[:4 + (4 if wild else 2) * L].cpu().numpy()
    logits.record_stream(self.stream)
    res = (host[4:4 + 2 * L].reshape(L, 2).copy(), float(host[:2].view(np.float64)[0]), int(host[2]))
    return res + (host[4 + 2 * L:].view(np.float64).copy(),) if wild else res

  def word_confidence(self, labels, space_id=None):
    """Word confidences (st_ctc_word_conf_f32; semantics: include/speecht_hip.h, tests/conf_oracle.py): for the given id lists,
    one per utterance of the batch, against the logits of the current shape
    -> (list of float64 arrays: log_conf of each word of the utterance -- ln of the probability that the stretch between the
    word's neighbouring spaces reads that word, the other words given, word boundaries summed out --, log_prob [B, 1] float64 =
    ln P(label), status [B]: != 0 where the label does not fit its utterance's frames -- then log_prob = -inf and the log_conf
    are NaN).  Words are the maximal runs of ids other than ``space_id`` (default: the vocabulary's space).
    Labels hold ids in [0, num_classes - 1) and at most MAX_ALIGN_LABELS of them."""
    from . import alignment, vocabulary
    lib = _lib.load()
    space_id = vocabulary.SPACE_ID if space_id is None else int(space_id)
    sh = self.shape
    xl = sh.X[-1]
    B, T = xl.batch, xl.frames
    if len(labels) != B:
      raise ValueError('word_confidence: {} label sequences for a batch of {}'.format(len(labels), B))
    lens = [len(l) for l in labels]
    offs = np.zeros(B + 1, dtype=np.int32)
    offs[1:] = np.cumsum(lens)
    N, max_len = int(offs[-1]), int(max(lens + [0]))
    if max_len > MAX_ALIGN_LABELS:
      raise ValueError('word_confidence: label of length {} is too long for the lattice kernel (max {})'.format(max_len, MAX_ALIGN_LABELS))
    ids = np.concatenate([np.asarray(l, dtype=np.int32).reshape(-1) for l in labels] + [np.zeros(1, np.int32)])
    # the kernel indexes LDS rows with the id: it must never see one outside the classes
    if N and (int(ids.min()) < 0 or int(ids.max()) >= self.num_classes - 1):
      raise ValueError('word_confidence: label ids must lie in [0, {}) (blank = {})'.format(self.num_classes - 1, self.num_classes - 1))
    if not 0 <= space_id < self.num_classes - 1:
      raise ValueError('word_confidence: space_id must lie in [0, {})'.format(self.num_classes - 1))
    runs = [alignment.word_runs(l, space_id) for l in labels]
    counts = [len(r) for r in runs]
    W = int(sum(counts))
    spans = np.array([(b, a, e) for b, r in enumerate(runs) for a, e in r] + [(0, 0, 0)], dtype=np.int32).reshape(-1)
    need = lib.st_ctc_word_conf_ws(B, T, max_len, B + W)
    ws = self._storage.view('conf_ws', need // 4 + 16, torch.int32)[0]
    # outputs in one buffer, one copy back: log_conf [W] | log_prob [B] (doubles) | status [B]
    out = self._storage.view('conf_out', 2 * (W + B) + B, torch.int32)[0]
    at = lambda first: ctypes.c_void_p(out.data_ptr() + 4 * first)
    d_ids, d_offs, d_spans = self._upload_i32(ids), self._upload_i32(offs), self._upload_i32(spans)
    self._wait_uploads()
    call('st_ctc_word_conf_f32', xl.ref, self._ptr(d_ids), self._ptr(d_offs), self._ptr(self.ctc_lens), max_len, space_id,
         self._ptr(d_spans), W, at(2 * W), at(0), at(2 * (W + B)), self._ptr(ws), ws.numel() * 4, self.stream_ptr)
    with torch.cuda.stream(self.stream):
      host = out[:2 * (W + B) + B].cpu().numpy()
    conf = host[:2 * W].view(np.float64)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return ([conf[first[b]:first[b + 1]].copy() for b in range(B)], host[2 * W:2 * (W + B)].view(np.float64).reshape(-1, 1).copy(),
            host[2 * (W + B):].copy())

  def spot(self, keywords, jobs=None, trace=False):
    """Keyword spotting (st_ctc_spot_f32; semantics: include/speecht_hip.h, tests/spot_oracle.py): the best occurrence of each
    keyword -- an id list, spaces allowed -- in the frames of each utterance, against the logits of the current shape.
    ``jobs``: [n, 2] (utterance, keyword) pairs; default: every pair, utterance-major.
    -> (score [n] float64: the log-likelihood ratio of reading the keyword on its best frames against the greedy reading of the
    same frames, <= 0, -inf where the keyword does not fit; spans [n, 2] int32: first output frame and one past the last, -1
    without a hit; status [n]: != 0 for a job outside the tables), in the order of ``jobs``.
    ``trace=True``: two more arrays, [n, T'] float64 and int32 -- for every frame the best score of the occurrences that end
    there and their first frame (-inf and -1 beyond the utterance): what `spotting.pick_hits` finds several hits in.

    One call of the kernel runs one states-per-lane lattice, so the jobs are grouped by the lattice their keyword needs (one
    long phrase does not put every short word on the 16-states-per-lane kernel) and, inside a group, ordered utterance-major:
    neighbouring workgroups then read the same rows.  Trace calls are split over jobs so that one call's trace stays under
    SPOT_TRACE_BYTES.  Keywords hold 1 .. MAX_SPOT_LABELS ids in [0, num_classes - 1)."""
    lib = _lib.load()
    sh = self.shape
    xl = sh.X[-1]
    B, T = xl.batch, xl.frames
    keywords = [np.asarray(k, dtype=np.int32).reshape(-1) for k in keywords]
    K = len(keywords)
    for k in keywords:
      if not 1 <= len(k) <= MAX_SPOT_LABELS:
        raise ValueError('spot: a keyword holds 1 .. {} ids, got {}'.format(MAX_SPOT_LABELS, len(k)))
      # the kernel indexes LDS rows with the id: it must never see one outside the classes
      if int(k.min()) < 0 or int(k.max()) >= self.num_classes - 1:
        raise ValueError('spot: keyword ids must lie in [0, {}) (blank = {})'.format(self.num_classes - 1, self.num_classes - 1))
    if jobs is None:
      jobs = np.stack(np.meshgrid(np.arange(B), np.arange(K), indexing='ij'), axis=-1)
    jobs = np.ascontiguousarray(jobs, dtype=np.int32).reshape(-1, 2)
    n = len(jobs)
    score = np.full(n, -np.inf)
    spans = np.full((n, 2), -1, dtype=np.int32)
    status = np.ones(n, dtype=np.int32)
    trace_score = np.full((n, T), -np.inf) if trace else None
    trace_start = np.full((n, T), -1, dtype=np.int32) if trace else None
    result = lambda: (score, spans, status) + ((trace_score, trace_start) if trace else ())
    if n == 0 or K == 0:
      return result()
    offs = np.zeros(K + 1, dtype=np.int32)
    offs[1:] = np.cumsum([len(k) for k in keywords])
    kpl_of = np.array([spot_lattice_kpl(len(k)) for k in keywords])
    known = (jobs[:, 1] >= 0) & (jobs[:, 1] < K)
    job_kpl = np.where(known, kpl_of[np.clip(jobs[:, 1], 0, K - 1)], SPOT_KPLS[0])      # (a job outside the tables: any lattice refuses it)
    d_ids, d_offs = self._upload_i32(np.concatenate(keywords)), self._upload_i32(offs)
    per_call = max(1, SPOT_TRACE_BYTES // (12 * T)) if trace else n
    for kpl in sorted(set(job_kpl.tolist())):
      group = np.flatnonzero(job_kpl == kpl)
      group = group[np.argsort(jobs[group, 0], kind='stable')]
      max_len = int(max([len(keywords[k]) for k in range(K) if kpl_of[k] == kpl]))
      need = lib.st_ctc_spot_ws(B, T, max_len, min(per_call, len(group)))
      ws = self._storage.view('spot_ws', need // 4 + 16, torch.int32)[0]
      for first in range(0, len(group), per_call):
        which = group[first:first + per_call]
        m = len(which)
        # outputs in one buffer, one copy back: score [m] | trace_score [m][T] (doubles) | span [m][2] | status [m] | trace_start [m][T]
        tr = m * T if trace else 0
        words = 2 * m + 2 * tr + 2 * m + m + tr
        out = self._storage.view('spot_out', words + 2, torch.int32)[0]
        at = lambda first_word: ctypes.c_void_p(out.data_ptr() + 4 * first_word)
        d_jobs = self._upload_i32(jobs[which].reshape(-1))
        self._wait_uploads()
        call('st_ctc_spot_f32', xl.ref, self._ptr(self.ctc_lens), self._ptr(d_ids), self._ptr(d_offs), K, max_len, self._ptr(d_jobs), m,
             at(0), at(2 * m + 2 * tr), at(2 * m) if trace else None, at(2 * m + 2 * tr + 3 * m) if trace else None,
             at(2 * m + 2 * tr + 2 * m), self._ptr(ws), ws.numel() * 4, self.stream_ptr)
        with torch.cuda.stream(self.stream):
          host = out[:words].cpu().numpy()
        score[which] = host[:2 * m].view(np.float64)
        spans[which] = host[2 * m + 2 * tr:2 * m + 2 * tr + 2 * m].reshape(m, 2)
        status[which] = host[2 * m + 2 * tr + 2 * m:2 * m + 2 * tr + 3 * m]
        if trace:
          trace_score[which] = host[2 * m:2 * m + 2 * tr].view(np.float64).reshape(m, T)
          trace_start[which] = host[2 * m + 2 * tr + 3 * m:].reshape(m, T)
    return result()

  def lm_beam_search_decode(self, lm, beam_width=100, input_transform='log10_softmax', lm_weight=0.8, word_count_weight=0.0,
                            valid_word_count_weight=2.3, oov_score=-1000.0):
    """The prefix beam search with a word n-gram scorer -- the reference's decoder (speech_model.py:84-111: beam 100,
    merge_repeated=False, on log10(softmax + 1e-8), lm_weight 0.8, word_count_weight 0.0, valid_word_count_weight 2.3) with an
    ARPA model (`language_model.LanguageModel`) in place of its KenLM scorer; semantics: tests/lm_oracle.py.
    -> (list of id lists, log_prob [B,1]); log_prob includes the LM terms."""
    lib = _lib.load()
    sh = self.shape
    B = sh.dec_lens.numel()
    need = lib.st_ctc_beam_ws(B, sh.t_out, int(beam_width))
    ws = self._storage.view('beam_ws', need // 4 + 16, torch.int32)[0]
    handle = lm.device_handle(self.device)
    self._wait_uploads()
    call('st_ctc_beam_search_decode_lm', sh.X[-1].ref, self._ptr(self.ctc_lens), int(beam_width), beam_input_transform(input_transform),
         handle, float(lm_weight), float(word_count_weight), float(valid_word_count_weight), float(oov_score),
         self._ptr(sh.dec_ids), sh.t_out, self._ptr(sh.dec_lens), self._ptr(sh.dec_score),
         self._ptr(ws), ws.numel() * 4, self.stream_ptr)
    lens = sh.dec_lens.cpu().numpy()
    ids = sh.dec_ids.view(-1, sh.t_out).cpu().numpy()
    return [ids[b, :lens[b]].tolist() for b in range(len(lens))], sh.dec_score.cpu().numpy().reshape(-1, 1)

  def _nbest_lists(self, n_best, beam_width, launch):
    """The N-best searches' buffers, one copy back and the lists: `launch(ids, T, lens, score, n_hyps, ws, ws_bytes)` issues the
    search on the engine's own stream (the serial path, like `align`)."""
    lib = _lib.load()
    sh = self.shape
    B, T, n = sh.dec_lens.numel(), sh.t_out, int(n_best)
    if not 1 <= n <= int(beam_width):
      raise ValueError('n_best must lie in 1..beam_width = {}, got {}'.format(int(beam_width), n))
    need = lib.st_ctc_beam_ws(B, T, int(beam_width))
    ws = self._storage.view('beam_ws', need // 4 + 16, torch.int32)[0]
    # outputs in one buffer, one copy back: ids [B][n][T] | lens [B][n] | log_prob [B][n] (float bits) | n_hyps [B]
    words = B * n * T + 2 * B * n + B
    out = self._storage.view('nbest_out', words + 2, torch.int32)[0]
    at = lambda first: ctypes.c_void_p(out.data_ptr() + 4 * first)
    self._wait_uploads()
    launch(at(0), T, at(B * n * T), at(B * n * T + B * n), at(B * n * T + 2 * B * n), self._ptr(ws), ws.numel() * 4)
    with torch.cuda.stream(self.stream):
      host = out[:words].cpu().numpy()
    ids = host[:B * n * T].reshape(B, n, T)
    lens = host[B * n * T:B * n * T + B * n].reshape(B, n)
    logp = host[B * n * T + B * n:B * n * T + 2 * B * n].view(np.float32).reshape(B, n)
    count = host[B * n * T + 2 * B * n:]
    return [[(ids[b, h, :min(lens[b, h], T)].tolist(), float(logp[b, h])) for h in range(count[b])] for b in range(B)]

  def _bias_tables(self, hotwords):
    """st_bias_tables of a `hotwords.Hotwords` on the engine's device -> (the struct by reference, what must stay alive)."""
    nxt, gain, fin = hotwords.device_tables(self.device)
    tables = _lib.BiasTables(nxt.data_ptr(), gain.data_ptr(), fin.data_ptr(), int(hotwords.n_states))
    return ctypes.byref(tables), (tables, nxt, gain, fin)

  def beam_search_decode_nbest(self, n_best, beam_width=16, input_transform=None, hotwords=None):
    """The N best final prefixes of ``beam_search_decode`` (st_ctc_beam_search_decode_nbest; ranking rules: include/speecht_hip.h,
    tests/nbest_oracle.py) -> per utterance a list of (ids, log_prob), best first, of min(n_best, entries alive) hypotheses;
    ``n_best=1`` returns the bits of ``beam_search_decode``.  merge_repeated is not offered: it could make two hypotheses equal.
    ``hotwords`` (a `hotwords.Hotwords`): the search biased towards its phrases (st_ctc_beam_search_decode_bias_nbest; log_prob then
    includes the bias, which `nbest.components` splits off); None is the unbiased code path."""
    code = beam_input_transform(input_transform)
    sh = self.shape
    if hotwords is not None:
      bias, keep = self._bias_tables(hotwords)
      return self._nbest_lists(n_best, beam_width, lambda ids, T, lens, score, count, ws, ws_bytes: call(
          'st_ctc_beam_search_decode_bias_nbest', sh.X[-1].ref, self._ptr(self.ctc_lens), int(beam_width), code, bias, int(n_best), ids,
          T, lens, score, count, ws, ws_bytes, self.stream_ptr))
    return self._nbest_lists(n_best, beam_width, lambda ids, T, lens, score, count, ws, ws_bytes: call(
        'st_ctc_beam_search_decode_nbest', sh.X[-1].ref, self._ptr(self.ctc_lens), int(beam_width), code, int(n_best), ids, T, lens,
        score, count, ws, ws_bytes, self.stream_ptr))

  def lm_beam_search_decode_nbest(self, lm, n_best, beam_width=100, input_transform='log10_softmax', lm_weight=0.8,
                                  word_count_weight=0.0, valid_word_count_weight=2.3, oov_score=-1000.0, hotwords=None):
    """The N best final prefixes of ``lm_beam_search_decode`` (st_ctc_beam_search_decode_lm_nbest): every final entry gains its
    end-of-utterance LM terms, then the entries are ranked by (total desc, rank in the beam asc) -> per utterance a list of
    (ids, log_prob), best first; log_prob includes the LM terms (`nbest.components` splits them off).  ``hotwords``: as
    ``beam_search_decode_nbest`` (st_ctc_beam_search_decode_lm_bias_nbest)."""
    code = beam_input_transform(input_transform)
    handle = lm.device_handle(self.device)
    sh = self.shape
    if hotwords is not None:
      bias, keep = self._bias_tables(hotwords)
      return self._nbest_lists(n_best, beam_width, lambda ids, T, lens, score, count, ws, ws_bytes: call(
          'st_ctc_beam_search_decode_lm_bias_nbest', sh.X[-1].ref, self._ptr(self.ctc_lens), int(beam_width), code, handle,
          float(lm_weight), float(word_count_weight), float(valid_word_count_weight), float(oov_score), bias, int(n_best), ids, T, lens,
          score, count, ws, ws_bytes, self.stream_ptr))
    return self._nbest_lists(n_best, beam_width, lambda ids, T, lens, score, count, ws, ws_bytes: call(
        'st_ctc_beam_search_decode_lm_nbest', sh.X[-1].ref, self._ptr(self.ctc_lens), int(beam_width), code, handle, float(lm_weight),
        float(word_count_weight), float(valid_word_count_weight), float(oov_score), int(n_best), ids, T, lens, score, count, ws,
        ws_bytes, self.stream_ptr))

  def lm_score_prefixes(self, lm, prefixes):
    """Sentence scores of id lists (ids 0..27: a-z ' space) under ``lm`` (st_lm_score_prefixes_f64; the definition:
    include/speecht_hip.h, tests/nbest_oracle.py) -> (G float64 [n]: the sum of the words' log10 n-gram probabilities plus </s>,
    n_words int32 [n], n_valid int32 [n]).  One lane per prefix, on the engine's own stream."""
    n = len(prefixes)
    if n == 0:
      return np.zeros(0), np.zeros(0, np.int32), np.zeros(0, np.int32)
    lens = np.array([len(p) for p in prefixes], dtype=np.int32)
    pitch = max(int(lens.max()), 1)
    ids = np.zeros((n, pitch), dtype=np.int32)
    for i, p in enumerate(prefixes):
      ids[i, :lens[i]] = p
    # (the kernel marks a prefix with an id outside 0..27 instead of failing the call: refuse it here)
    if int(ids.min()) < 0 or int(ids.max()) > 27:
      raise ValueError('lm_score_prefixes: ids must lie in 0..27 (a-z, apostrophe, space)')
    handle = lm.device_handle(self.device)
    # outputs in one buffer, one copy back: G [n] (doubles) | n_words [n] | n_valid [n]
    out = self._storage.view('lm_score_out', 4 * n + 2, torch.int32)[0]
    at = lambda first: ctypes.c_void_p(out.data_ptr() + 4 * first)
    d_ids, d_lens = self._upload_i32(ids.reshape(-1)), self._upload_i32(lens)
    self._wait_uploads()
    call('st_lm_score_prefixes_f64', handle, self._ptr(d_ids), pitch, self._ptr(d_lens), n, at(0), at(2 * n), at(3 * n), self.stream_ptr)
    with torch.cuda.stream(self.stream):
      host = out[:4 * n].cpu().numpy()
    return host[:2 * n].view(np.float64).copy(), host[2 * n:3 * n].copy(), host[3 * n:].copy()

  def lm_beam_search_decode_candidates(self, lm, weights, beam_width=100, input_transform='log10_softmax', oov_score=-1000.0,
                                       max_workspace_bytes=CANDIDATE_WORKSPACE_BYTES):
    """``lm_beam_search_decode`` for several weight triples on the same logits (the LM weight search's generation):
    ``weights`` is a sequence of (lm_weight, word_count_weight, valid_word_count_weight).  The log-softmax rows are computed once
    per call and one launch decodes every (candidate, utterance) pair (st_ctc_beam_search_decode_lm_candidates).  Candidates
    are split into calls whose workspace stays under ``max_workspace_bytes`` (at least one candidate per call); the split does
    not change any result: candidate p's outputs are bit-identical to ``lm_beam_search_decode`` with p's weights.
    -> `CandidateDecodes`: the device outputs (ids [P, B, T], lens [P, B], log_prob [P, B]) and, on demand, a host view."""
    lib = _lib.load()
    w = np.asarray(weights, dtype=np.float32).reshape(-1, 3)
    sh = self.shape
    P, B, T = len(w), sh.dec_lens.numel(), sh.t_out
    if P < 1:
      raise ValueError('lm_beam_search_decode_candidates: at least one weight triple')
    if not np.all(np.isfinite(w)):
      raise ValueError('lm_beam_search_decode_candidates: weights must be finite')
    chunk = P
    while chunk > 1 and lib.st_ctc_beam_lm_candidates_ws(B, T, int(beam_width), chunk) > max_workspace_bytes:
      chunk = (chunk + 1) // 2
    need = lib.st_ctc_beam_lm_candidates_ws(B, T, int(beam_width), chunk)
    ws = self._storage.view('beam_ws', need // 4 + 16, torch.int32)[0]
    ids = torch.zeros(P * B * T, dtype=torch.int32, device=self.device)
    lens = torch.empty(P * B, dtype=torch.int32, device=self.device)
    logp = torch.empty(P * B, dtype=torch.float32, device=self.device)
    handle = lm.device_handle(self.device)
    code = beam_input_transform(input_transform)
    self._wait_uploads()
    for p0 in range(0, P, chunk):
      n = min(chunk, P - p0)
      wc = np.ascontiguousarray(w[p0:p0 + n])
      call('st_ctc_beam_search_decode_lm_candidates', sh.X[-1].ref, self._ptr(self.ctc_lens), int(beam_width), code, handle,
           wc.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), n, float(oov_score),
           ctypes.c_void_p(ids.data_ptr() + 4 * p0 * B * T), T, ctypes.c_void_p(lens.data_ptr() + 4 * p0 * B),
           ctypes.c_void_p(logp.data_ptr() + 4 * p0 * B), self._ptr(ws), ws.numel() * 4, self.stream_ptr)
    return CandidateDecodes(ids.view(P, B, T), lens.view(P, B), logp.view(P, B), self.stream)

  def lm_beam_search_decode_async(self, lm, beam_width=100, decode_stream=None, input_transform='log10_softmax', lm_weight=0.8,
                                  word_count_weight=0.0, valid_word_count_weight=2.3, oov_score=-1000.0):
    """``lm_beam_search_decode`` on the decoder streams, like ``beam_search_decode_async``: returns a handle whose ``result()``
    waits for this batch only."""
    handle = lm.device_handle(self.device)
    code = beam_input_transform(input_transform)

    def launch(desc, lens, ids, T, out_lens, score, ws, ws_bytes, stream):
      call('st_ctc_beam_search_decode_lm', desc, lens, int(beam_width), code, handle, float(lm_weight), float(word_count_weight),
           float(valid_word_count_weight), float(oov_score), ids, T, out_lens, score, ws, ws_bytes, stream)
    return self._beam_decode_async(beam_width, decode_stream, launch)

  def beam_search_decode_async(self, beam_width=16, decode_stream=None, input_transform=None):
    """``beam_search_decode`` without the host synchronisation and OFF the compute stream: the logits and lengths of this
    batch are copied into a decoder slot, the search runs on ``decode_stream`` (default: a stream of the engine's own;
    `decoder_streams` gives CU-masked ones -- a list of streams is used in turn, consecutive batches' searches then run side by
    side) and its outputs go to pinned host memory; returns a handle whose
    ``result()`` waits for this batch only.  The caller enqueues the next batch's forward pass meanwhile -- the search is ONE
    wavefront per utterance (3.9 ms for 16 x 30 s, beam 16: as long as the forward pass) and leaves the chip to it."""
    code = beam_input_transform(input_transform)

    def launch(desc, lens, ids, T, out_lens, score, ws, ws_bytes, stream):
      call('st_ctc_beam_search_decode_ex', desc, lens, int(beam_width), code, ids, T, out_lens, score, ws, ws_bytes, stream)
    return self._beam_decode_async(beam_width, decode_stream, launch)

  def _beam_decode_async(self, beam_width, decode_stream, launch):
    """The slot ring of the asynchronous beam searches; `launch` issues the search itself on the decoder stream."""
    lib = _lib.load()
    B, T = self.shape.dec_lens.numel(), self.shape.t_out
    xl = self.shape.X[-1]
    need = lib.st_ctc_beam_ws(B, T, int(beam_width))
    streams = list(decode_stream) if isinstance(decode_stream, (list, tuple)) else [decode_stream]
    # one slot more than decoder streams: the forward pass fills a slot while every stream searches one
    if len(self._beam_slots) != len(streams) + 1:
      for old in self._beam_slots:
        if old is not None:
          old['event'].synchronize()
      self._beam_slots, self._beam_turn = [None] * (len(streams) + 1), 0
    self._beam_turn += 1
    which = self._beam_turn % len(self._beam_slots)
    slot = self._beam_slots[which]
    decode_stream = streams[self._beam_turn % len(streams)]
    main = self.stream
    if decode_stream is None:
      if self._decode_stream is None:
        self._decode_stream = torch.cuda.Stream(self.device)
      decode_stream = self._decode_stream
    if slot is None or slot['logits'].numel() < xl.buf.numel() or slot['ids'].numel() < B * T or slot['ws'].numel() * 4 < need or \
        slot['lens'].numel() < B:
      if slot is not None:
        slot['event'].synchronize()                               # the old buffers may still be in use
      i32 = lambda n, **kw: torch.empty(max(n, 1), dtype=torch.int32, **kw)
      slot = dict(logits=torch.empty(xl.buf.numel(), dtype=torch.float32, device=self.device), lens=i32(B, device=self.device),
                  ids=i32(B * T, device=self.device), out_lens=i32(B, device=self.device),
                  score=torch.empty(max(B, 1), dtype=torch.float32, device=self.device), ws=i32(need // 4 + 16, device=self.device),
                  ids_h=i32(B * T, pin_memory=True), lens_h=i32(B, pin_memory=True),
                  score_h=torch.empty(max(B, 1), dtype=torch.float32, pin_memory=True), event=torch.cuda.Event(), generation=0)
      slot['event'].record(decode_stream)
      self._beam_slots[which] = slot
    slot['generation'] += 1                                       # handles of the batch that last used this slot are stale from here on
    self._wait_uploads()
    main.wait_event(slot['event'])                               # the search that last read this slot is through
    with torch.cuda.stream(main):
      slot['logits'][:xl.buf.numel()].copy_(xl.buf, non_blocking=True)
      slot['lens'][:B].copy_(self.ctc_lens, non_blocking=True)
      ready = torch.cuda.Event()
      ready.record(main)
    desc = Tensor3(slot['logits'].data_ptr(), xl.batch, xl.frames, xl.channels, xl.halo, xl.t_pitch, xl.c_pitch)
    decode_stream.wait_event(ready)
    launch(ctypes.byref(desc), self._ptr(slot['lens']), self._ptr(slot['ids']), T, self._ptr(slot['out_lens']), self._ptr(slot['score']),
           self._ptr(slot['ws']), slot['ws'].numel() * 4, ctypes.c_void_p(decode_stream.cuda_stream))
    with torch.cuda.stream(decode_stream):
      slot['ids_h'][:B * T].copy_(slot['ids'][:B * T], non_blocking=True)
      slot['lens_h'][:B].copy_(slot['out_lens'][:B], non_blocking=True)
      slot['score_h'][:B].copy_(slot['score'][:B], non_blocking=True)
      slot['event'].record(decode_stream)
    return _PendingBeamDecode(slot, B, T)
