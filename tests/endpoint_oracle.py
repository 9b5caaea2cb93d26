"""The specification of endpointing for live streams (csrc/stream_endpoint_core.h, st_ctc_greedy_endpoint_stream,
st_stream_endpoint_host), in plain Python and float64.

The rule is a pure function of a stream's logits rows.  Row t is SILENT when its argmax -- first maximum on ties, columns below
``num_classes`` only -- is the blank (C - 1) or ``space_id`` (-1: no such class), SPEECH otherwise.  With R = silence_frames >= 1,
L = lead_frames >= 1, M = max_frames >= L and the state (u0, started, run): row t always joins the open utterance; a speech row sets
started and run = 0, a silent row increments run; then, with len = t + 1 - u0, the first of

  1 (silence)  started and run >= R      the utterance [u0, t + 1) is final
  2 (length)   started and len >= M      final as well
  3 (discard)  not started and len >= L  no utterance, the rows are dropped

that applies fires, and after any event u0 = t + 1, started = False, run = 0.  At the end of the stream (``limit`` rows consumed) a
non-empty open stretch ends with event 4 if it has started and with event 3 otherwise.

`segment` is the rule on a whole stream.  `Spec` derives from its result -- never from a walk over steps -- what a step that consumes
the frames [a, b) must write: events, pieces, ids, the carried state.  The device works the other way round (a walk that carries
state), so agreement for every cut says the walk loses nothing at a step boundary."""
import numpy as np

SILENCE, LENGTH, DISCARD, END = 1, 2, 3, 4
FINAL_KINDS = (SILENCE, LENGTH, END)
UNUSED = (0, 0, -1, 0)


def argmax_rows(logits, num_classes):
  """(class, value) per row: first maximum on ties, columns below ``num_classes`` only."""
  x = np.asarray(logits)[:, :num_classes]
  k = np.argmax(x, axis=1) if len(x) else np.zeros(0, np.int64)     # (numpy returns the first maximum)
  return k.astype(np.int64), x[np.arange(len(x)), k]


def silent_rows(logits, num_classes, space_id=-1):
  k, _ = argmax_rows(logits, num_classes)
  return (k == num_classes - 1) | ((k == space_id) if space_id >= 0 else False)


def pieces_needed(n, R, L, M):
  """Piece (and event) slots per stream for steps of at most ``n`` >= 1 rows per stream."""
  return 2 + (n - 1) // min(L, R + 1, M)


def segment(silent, R, L, M, finished=True):
  """The rule on the rows ``silent`` (bool per row) -> [(kind, u0, end, first_speech, last_speech, index)]: first / last speech are -1 in a
  discard; index counts the finals, a discard carries the index the next final will get."""
  assert R >= 1 and L >= 1 and M >= L
  events, u0, started, run, first, last, index = [], 0, False, 0, -1, -1, 0
  for t, quiet in enumerate(silent):
    if quiet:
      run += 1
    else:
      if not started:
        started, first = True, t
      last, run = t, 0
    n = t + 1 - u0
    kind = (SILENCE if run >= R else LENGTH if n >= M else 0) if started else (DISCARD if n >= L else 0)
    if kind:
      events.append((kind, u0, t + 1, first, last, index))
      index += kind != DISCARD
      u0, started, run, first, last = t + 1, False, 0, -1, -1
  if finished and len(silent) > u0:
    events.append((END if started else DISCARD, u0, len(silent), first, last, index))
  return events


def collapse(k, blank, last=-1):
  """Greedy CTC on the argmax ids ``k``: repeats merged, blanks dropped; ``last``: the id before the first row."""
  out = []
  for c in k:
    c = int(c)
    if c != blank and c != last:
      out.append(c)
    last = c
  return out


class Spec:
  """One stream of ``limit`` consumed rows (default: all of ``logits``)."""

  def __init__(self, logits, num_classes, space_id, R, L, M, limit=None):
    limit = len(logits) if limit is None else min(int(limit), len(logits))
    self.C, self.blank, self.R, self.L, self.M, self.limit = num_classes, num_classes - 1, R, L, M, limit
    self.k, self.v = argmax_rows(np.asarray(logits)[:limit], num_classes)
    self.silent = (self.k == self.blank) | ((self.k == space_id) if space_id >= 0 else False)
    self.row_events = segment(self.silent, R, L, M, finished=False)
    self.events = segment(self.silent, R, L, M, finished=True)

  def finals(self):
    return [e for e in self.events if e[0] in FINAL_KINDS]

  def neg_sum(self, u0, end):
    """The negative sum of the chosen logits of rows [u0, end) in the whole-utterance greedy decoder's order: row i of the stretch is
    added, in float32 and in row order, to slot i % 256; the slots are summed as a binary tree of neighbours."""
    slots = np.zeros(256, np.float32)
    for i, x in enumerate(self.v[u0:end]):
      slots[i % 256] = np.float32(slots[i % 256] + np.float32(x))
    while len(slots) > 1:
      slots = (slots[0::2] + slots[1::2]).astype(np.float32)
    return np.float32(-slots[0])

  def open_at(self, b, closed=False):
    """Start of the stretch that is open once the frames below ``b`` are consumed."""
    ends = [e[2] for e in (self.events if closed else self.row_events) if e[2] <= b]
    return ends[-1] if ends else 0

  def state(self, b, finishing=False):
    """The carried record {u0, started, run, first_speech, last_speech, finals so far, last argmax id, rows consumed} and the open
    stretch's negative sum after a step that ends at frame ``b``."""
    u0 = self.open_at(b, closed=finishing)
    speech = np.flatnonzero(~self.silent[u0:b]) + u0
    started = len(speech) > 0
    run = (b - 1 - speech[-1]) if started else b - u0
    index = sum(1 for e in (self.events if finishing else self.row_events) if e[2] <= b and e[0] in FINAL_KINDS)
    last = int(self.k[b - 1]) if b > u0 else -1
    first_s, last_s = (int(speech[0]), int(speech[-1])) if started else (-1, -1)
    return (u0, int(started), int(run), first_s, last_s, index, last, b), self.neg_sum(u0, b)

  def step(self, a, b, first_row, reset, finishing, P):
    """A step that consumes the frames [a, b), the stream's rows starting at row ``first_row`` of the launch; ``reset``: the host's
    flag (a == 0); ``finishing``: b is the limit.  -> dict(events [n][8], pieces [P][4], ids, state, neg_sum)."""
    assert 0 <= a <= b <= self.limit and (not finishing or b == self.limit) and (not reset or a == 0)
    pieces, ids, events = [], [], []

    def rows_of(u0, hi, limit):                                     # the step's rows of the stretch that starts at u0: [max(u0, a), hi)
      lo = max(u0, a)
      ids.extend(collapse(self.k[lo:hi], self.blank, int(self.k[lo - 1]) if lo > u0 else -1))
      pieces.append((first_row + lo - a, hi - lo, limit, int(u0 > a or (bool(reset) and u0 == a))))

    def event(e):
      kind, u0, end, fs, ls, index = e
      events.append([kind, u0, end, fs, ls, len(ids), int(self.neg_sum(u0, end).view(np.int32)), index])

    for e in self.row_events:
      if a < e[2] <= b:                                             # an event on a row of this step closes a stretch with rows in it
        rows_of(e[1], e[2], e[2] if e[0] in FINAL_KINDS else -1)
        event(e)
    tail = self.open_at(b)                                          # the stretch still open after the step's last row ...
    closing = self.events[len(self.row_events):] if finishing else []   # ... which the end of the stream closes, unless it is empty
    if tail < b and a < b:
      rows_of(tail, b, b if closing and closing[0][0] == END else -1)
    elif (tail == b and a < b) or (reset and a == b):
      pieces.append((0, 0, -1, 1))                                  # an event on the step's last row, or a fresh stream without rows
    elif closing and closing[0][0] == END:
      pieces.append((0, 0, b, 0))                                   # a final whose rows all came in earlier steps
    for e in closing:
      event(e)
    assert len(pieces) <= P and len(events) <= P, (len(pieces), len(events), P)
    state, neg = self.state(b, finishing)
    return dict(events=events, pieces=pieces + [UNUSED] * (P - len(pieces)), ids=ids, state=state, neg_sum=neg)
