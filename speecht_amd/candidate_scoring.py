"""Letter / word error statistics of several decodings of one batch at once -- one `EvalStatistics` per LM-weight candidate,
exactly what ``Evaluation.run_step(..., save=False, verbose=False)`` gives for that candidate's decodings.

The pairing of labels with decodings is ``run_step``'s: the reference walk by default (``Evaluation.extract_decoded_ids``, its
quirk included: an empty decoding yields nothing and shifts the pairs behind it, and running out of decodings raises the same
RuntimeError), rows with ``pair_by_row``.  The pairing needs only the decodings' lengths; the edit distances of all pairs of all
candidates come from one launch of the device kernel (st_edit_distance_pairs) on the decodings the multi-candidate beam search
left on the device.  The rates and sums go through ``EvalStatistics.track_distances``, the arithmetic of ``track_decoding``, in
the order ``run_step`` tracks them, so the statistics are bit-identical to the host path (``device=False``), which runs
``track_decoding`` itself on the decoded strings.  A pair the kernel refuses (an id outside 0..27, a sequence longer than
st_edit_distance_max_len()) is scored on the host."""
import ctypes

import numpy as np

from . import _lib, editdistance, vocabulary
from .evaluation import EvalStatistics, Evaluation

_EMPTY_WARNING = ('warning: {} decoding(s) of this batch are empty; the reference pairing (evaluation.py:144-151) skips them, '
                  'so later expected/decoded pairs are shifted -- pass --pair-by-row to pair by utterance')
_RAN_OUT = ('ran out of decodings before labels: an utterance of this batch decoded to the empty string and '
            'the reference\'s lock-step pairing (evaluation.py:144-151) cannot continue; use --pair-by-row')


def walk_rows(row_lengths):
  """``Evaluation.extract_decoded_ids`` on a sparse tensor whose rows have these lengths, yielding the ROW INDEX of every id list
  it would yield (row 0 when that row is empty and a later row starts it off, the last non-empty row at the end)."""
  current_row = 0
  for b, n in enumerate(row_lengths):
    if n > 0 and b > current_row:
      yield current_row
      current_row = b
  yield current_row


def pairings(label, decoded_lens, pair_by_row=False, warn=True):
  """-> (label id lists in pairing order, [per candidate: list of (label index, decoded row)]) for the label sparse tensor of
  a batch and the decoded lengths [P][B]; raises RuntimeError where ``run_step`` would."""
  if pair_by_row:
    labels = Evaluation.rows_by_batch(label)
  else:
    labels = list(Evaluation.extract_decoded_ids(label))
  out = []
  for lens in decoded_lens:
    lens = [int(n) for n in lens]
    if pair_by_row:
      rows = iter(range(len(lens)))
    else:
      rows = walk_rows(lens)
      empty = sum(1 for n in lens if n == 0)
      if empty and warn:
        print(_EMPTY_WARNING.format(empty))
    pairs = []
    for k in range(len(labels)):
      try:
        pairs.append((k, next(rows)))
      except StopIteration:
        raise RuntimeError(_RAN_OUT) from None
    out.append(pairs)
  return labels, out


def score_candidates(label, decodes, pair_by_row=False, device=True):
  """One `EvalStatistics` per candidate of ``decodes`` (engine_decode.CandidateDecodes) against the labels of the batch
  (the sparse tensor ``model.step(return_label=True)`` gives).  ``device=False``: the host path, ``track_decoding`` on the
  strings."""
  import torch
  P, B, T = decodes.ids.shape
  lens = decodes.lens_host()
  labels, per_candidate = pairings(label, lens, pair_by_row)
  expected = [vocabulary.ids_to_sentence(ids) for ids in labels]
  stats = [EvalStatistics() for _ in range(P)]
  if not device:
    host = decodes.host()
    for p in range(P):
      for k, b in per_candidate[p]:
        stats[p].track_decoding(vocabulary.ids_to_sentence(host[p][0][b]), expected[k])
    return stats
  lib = _lib.load()
  max_len = lib.st_edit_distance_max_len()
  on_device = [all(0 <= int(v) <= vocabulary.SPACE_ID for v in ids) and len(ids) <= max_len for ids in labels]
  pitch = max([len(ids) for ids in labels] + [1])
  mat = np.zeros((max(len(labels), 1), pitch), dtype=np.int32)
  lab_lens = np.zeros(max(len(labels), 1), dtype=np.int32)
  for k, ids in enumerate(labels):
    if on_device[k]:
      mat[k, :len(ids)] = ids
      lab_lens[k] = len(ids)
  flat = [(k, p * B + b) for p in range(P) for k, b in per_candidate[p]]
  dist = np.full((len(flat), 2), -1, dtype=np.int32)
  if flat:
    dev = decodes.ids.device
    stream = decodes.stream
    with torch.cuda.stream(stream):
      d_mat = torch.as_tensor(mat).to(dev, non_blocking=False)
      d_lab_lens = torch.as_tensor(lab_lens).to(dev)
      d_pairs = torch.as_tensor(np.asarray(flat, dtype=np.int32)).to(dev)
      d_out = torch.empty(len(flat) * 2, dtype=torch.int32, device=dev)
      _lib.call('st_edit_distance_pairs', ctypes.c_void_p(d_mat.data_ptr()), len(labels), pitch, ctypes.c_void_p(d_lab_lens.data_ptr()),
                ctypes.c_void_p(decodes.ids.data_ptr()), P * B, T, ctypes.c_void_p(decodes.lens.data_ptr()),
                ctypes.c_void_p(d_pairs.data_ptr()), len(flat), ctypes.c_void_p(d_out.data_ptr()), ctypes.c_void_p(stream.cuda_stream))
      dist = d_out.cpu().numpy().reshape(-1, 2)
  i = 0
  for p in range(P):
    for k, b in per_candidate[p]:
      led, wed = int(dist[i, 0]), int(dist[i, 1])
      exp = expected[k]
      if not on_device[k] or led < 0:
        hyp = vocabulary.ids_to_sentence(decodes.ids[p, b, :min(int(lens[p, b]), T)].cpu().tolist())
        led, wed = editdistance.eval(exp, hyp), editdistance.eval(exp.split(), hyp.split())
      stats[p].track_distances(led, wed, len(exp), len(exp.split()))
      i += 1
  return stats
