"""Partial transcripts for training: labels that leave audio out, marked with a wildcard (DESIGN.md "Training on partial
transcripts").  ``PartialTranscripts.apply`` turns the label lists of a training batch into lists that may hold
``WILDCARD``, which ``Wav2LetterEngine.set_labels(..., wildcard=True)`` uploads and ``ctc_loss_grad`` scores with
st_ctc_loss_grad_wild_f32: a wildcard state emits e^bias times the frame's summed label probability.

Three sources of wildcards, all applied to the ids the preprocessing cache already holds (no re-run of ``preprocess``):

  token   the transcript's own marks: the cache stores a character outside the vocabulary as ``ord - 97`` (`vocabulary`), '*'
          as -55; a run of ids equal to ``sentence_to_ids(token)`` that stands as a word of its own -- between spaces or at an end
          -- becomes one WILDCARD.  Every OTHER id outside [0, SIZE) is refused first: a back-tick is -1 and would otherwise be
          read as WILDCARD itself.
  ends    a wildcard and a space before every label and a space and a wildcard after it (recordings that open and close with
          words the text lacks).
  drop    the experiment that makes the feature usable on a fully labelled corpus: every word is replaced by a wildcard with
          probability P, runs of replaced words collapse into one wildcard, never every word of a transcript.

The defaults (bias -1.0 nats per frame, drop 0) are guesses that nobody has tuned on data.

Randomness is counter-based (Philox): an utterance's draws are a function of (seed, draw id) alone, the draw id being
``augmentation.draw_ids`` -- step * global batch + row in the global batch -- so they are the same under data parallelism and
after a resume, as with SpecAugment."""
import numpy as np

from . import vocabulary

WILDCARD = -1                  # engine_decode.WILDCARD (kept here so that this module imports without torch)
WILDCARD_TOKEN = '*'
WILDCARD_BIAS = -1.0           # nats per frame: a guess, not tuned on data
REFUSED = -2                   # what a refused label becomes in deferred mode: an id that no engine accepts


def draw_ids(global_step, batch, world=1, rank=0):
  """augmentation.draw_ids (restated: that module binds the native library)."""
  return np.int64(global_step) * np.int64(batch * world) + np.int64(rank * batch) + np.arange(batch, dtype=np.int64)


def _words(ids):
  """The label as words: lists of ids between spaces (empty words where spaces meet or stand at an end)."""
  words = [[]]
  for i in ids:
    if i == vocabulary.SPACE_ID:
      words.append([])
    else:
      words[-1].append(i)
  return words


def _join(words):
  out = []
  for k, w in enumerate(words):
    out += ([vocabulary.SPACE_ID] if k else []) + list(w)
  return out


def _collapse(words):
  """Neighbouring wildcard words become one."""
  out = []
  for w in words:
    if w == [WILDCARD] and out and out[-1] == [WILDCARD]:
      continue
    out.append(w)
  return out


class PartialTranscripts:
  """token: how transcripts write the wildcard (None: they do not); ends: wrap every label; bias: the wildcard's price per
  frame in nats, <= 0; drop: the probability a word is replaced; seed: of the drop draws."""

  def __init__(self, token=WILDCARD_TOKEN, ends=False, bias=WILDCARD_BIAS, drop=0.0, seed=0):
    if token is not None:
      ids = vocabulary.sentence_to_ids(token)
      if not ids or vocabulary.SPACE_ID in ids or all(0 <= i < vocabulary.SIZE for i in ids):
        raise ValueError('the wildcard token must be a word outside the vocabulary, not {!r}'.format(token))
    self.token = token
    self.token_ids = vocabulary.sentence_to_ids(token) if token is not None else None
    self.ends = bool(ends)
    self.bias = float(bias)
    if not (np.isfinite(self.bias) and self.bias <= 0.0):
      raise ValueError('wildcard bias must be finite and <= 0, not {}'.format(bias))
    self.drop = float(drop)
    if not 0.0 <= self.drop < 1.0:
      raise ValueError('wildcard drop must lie in [0, 1), not {}'.format(drop))
    self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF

  def __repr__(self):
    return 'PartialTranscripts(token={!r}, ends={}, bias={:g}, drop={:g}, seed={})'.format(self.token, self.ends, self.bias, self.drop,
                                                                                         self.seed)

  def mark(self, ids):
    """One label: token words -> WILDCARD, after refusing every other id outside the vocabulary -> words.  Without a token
    (``token_ids`` None) no word is one, and every id is checked."""
    words = _words([int(i) for i in ids])
    rest = [i for w in words if w != self.token_ids for i in w]
    if any(not 0 <= i < vocabulary.SIZE for i in rest):
      bad = sorted({i for i in rest if not 0 <= i < vocabulary.SIZE})
      raise ValueError('label ids must lie in [0, {}) or spell the wildcard token {!r} as a word of its own; got {} ({})'.format(
          vocabulary.SIZE, self.token, bad, ', '.join(repr(vocabulary.id_to_letter(i)) for i in bad)))
    return _collapse([[WILDCARD] if w == self.token_ids else w for w in words])

  def dropped(self, words, draw_id):
    """Words replaced at probability ``drop``; the draws are a function of (seed, draw id).  At least one word stays."""
    real = [k for k, w in enumerate(words) if w and w != [WILDCARD]]
    if self.drop <= 0.0 or not real:
      return words
    u = np.random.Generator(np.random.Philox(key=[self.seed, int(draw_id) & 0xFFFFFFFFFFFFFFFF])).random(len(real) + 1)
    gone = [k for k, x in zip(real, u[1:]) if x < self.drop]
    if len(gone) == len(real):
      gone.remove(real[min(int(u[0] * len(real)), len(real) - 1)])
    gone = set(gone)
    return _collapse([[WILDCARD] if k in gone else w for k, w in enumerate(words)])

  def apply(self, label_lists, step=0, rank=0, world=1, defer=False):
    """The labels of one rank's batch at one step -> lists of ids that may hold WILDCARD.  ``defer`` (data parallelism, where
    raising on one rank would leave the others waiting): a refused label comes back as [REFUSED], which the engine's own
    deferred check turns into status 2 on every rank together."""
    ids = draw_ids(step, len(label_lists), world, rank)
    out = []
    for label, draw in zip(label_lists, ids):
      try:
        words = self.mark(label)                     # (also without a token: the range check is not the token's)
      except ValueError:
        if not defer:
          raise
        out.append([REFUSED])
        continue
      words = self.dropped(words, draw)
      if self.ends:
        words = _collapse([[WILDCARD]] + ([] if words == [[]] else words) + [[WILDCARD]])     # (the empty label: one wildcard)
      out.append(_join(words))
    return out


def drop_probability(value):
  """The argparse type of --wildcard-drop: a number in [0, 1)."""
  import argparse
  try:
    drop = float(value)
  except ValueError:
    drop = float('nan')
  if not 0.0 <= drop < 1.0:
    raise argparse.ArgumentTypeError('expected a probability in [0, 1), got {!r}'.format(value))
  return drop


def add_arguments(parser, bias_type=float):
  """The `speecht-cli train` flags."""
  import argparse
  parser.add_argument('--wildcard', dest='wildcard', type=str, nargs='?', const=WILDCARD_TOKEN, default=argparse.SUPPRESS, metavar='TOKEN',
                      help='(extension) train on partial transcripts: TOKEN (default "*") as a word of its own in a transcript stands '
                           'for audio the text leaves out and becomes a wildcard label of the CTC loss, which emits the frame\'s '
                           'summed label probability at a price.  Works on the cached transcripts; evaluation stays plain')
  parser.add_argument('--wildcard-ends', dest='wildcard_ends', action='store_true', default=argparse.SUPPRESS,
                      help='put a wildcard before and after every transcript (implies --wildcard): recordings that open and close '
                           'with words the text lacks')
  parser.add_argument('--wildcard-bias', dest='wildcard_bias', type=bias_type, default=argparse.SUPPRESS, metavar='X',
                      help='what a frame given to a wildcard costs, in nats, <= 0 (implies --wildcard; default -1.0: a guess, nobody '
                           'has tuned it on data)')
  parser.add_argument('--wildcard-drop', dest='wildcard_drop', type=drop_probability, default=argparse.SUPPRESS, metavar='P',
                      help='replace every word of every training transcript by a wildcard with probability P, anew at every step '
                           '(implies --wildcard; default 0, untuned): the experiment on a fully labelled corpus.  Draws follow '
                           '--augment-seed / --seed')


def from_flags(flags):
  """The PartialTranscripts the train flags ask for, or None when none of them is given."""
  given = [f for f in ('wildcard', 'wildcard_ends', 'wildcard_bias', 'wildcard_drop') if hasattr(flags, f)]
  if not given:
    return None
  seed = getattr(flags, 'augment_seed', None)
  if seed is None:
    seed = getattr(flags, 'seed', None) or 0
  bias = getattr(flags, 'wildcard_bias', None)
  return PartialTranscripts(token=getattr(flags, 'wildcard', None) or WILDCARD_TOKEN, ends=bool(getattr(flags, 'wildcard_ends', False)),
                            bias=WILDCARD_BIAS if bias is None else bias, drop=getattr(flags, 'wildcard_drop', 0.0) or 0.0, seed=seed)
