"""Inputs and the step driver the endpointing tests share (tests/test_endpoint_host.py on the host form, tests/test_gpu_endpoint.py on
the kernel): seeded streams of silent / speech rows with exact ties, cut into steps in many ways, every step's events, pieces, ids
and carried state held to tests/endpoint_oracle.py."""
import ctypes
import itertools

import numpy as np

from tests import endpoint_oracle as EO

PITCH = 32
POISON = 9.0                 # in the columns at and past C: larger than every logit, so a kernel that looked there would pick it
CUTS = (1, 2, 7, 10, 80)
PARAMS = [(R, L, M) for R in (1, 2, 5) for L in (1, 3, 7) for M in sorted({L, 9, 40}) if M >= L]
CLASSES = (2, 5, 29, 32)
# what a sweep must have met: an event on the first and on the last row of a step, two in one step, the ways a stream can finish
SITUATIONS = ('first_row', 'last_row', 'two_events', 'finish_started', 'finish_unstarted', 'finish_without_rows', 'rows_past_limit')


def stream_logits(seed, T, C, space_id, R, L, M):
  """[T, C] float32: stretches of silence and speech whose lengths straddle R, L and M, so that all three events occur; some rows are
  exact ties -- blank = a label (the label, the lower index, wins: speech), space = blank (space wins: silent either way)."""
  rng = np.random.RandomState(seed)
  blank = C - 1
  labels = [c for c in range(C) if c != blank and c != space_id]
  silent_ids = [blank] + ([space_id] if space_id >= 0 else [])
  x = rng.standard_normal((T, C)).astype(np.float32)
  t, quiet = 0, bool(seed % 2)
  while t < T:
    span = int(rng.choice([1, R - 1, R, R + 1, L - 1, L, L + 1, M - 1, M, M + 3, 2])) if quiet else int(rng.choice([1, 2, 3, M // 2 + 1, M + 2]))
    span = max(span, 1)
    for j in range(t, min(t + span, T)):
      pool = silent_ids if (quiet or not labels) else labels
      c = pool[rng.randint(len(pool))]
      top = np.float32(x[j].max() + 1.0)
      x[j, c] = top
      roll = rng.randint(8)
      if roll == 0 and labels and c == blank:
        x[j, labels[rng.randint(len(labels))]] = top               # blank = label: the label wins, the row is speech
      elif roll == 1 and space_id >= 0 and c in silent_ids:
        x[j, blank] = x[j, space_id] = top                         # space = blank: silent either way
    t += span
    quiet = not quiet
  return x


def make_streams(seed, S, C, space_id, R, L, M, T=120):
  """S streams: logits [T, C], consumed lengths (rows at or past them are offered and must not be taken), one stream of length 0."""
  rng = np.random.RandomState(1000 + seed)
  logits = [stream_logits(seed * 31 + s, T, C, space_id, R, L, M) for s in range(S)]
  lens = [int(rng.randint(T // 2, T - 3)) for _ in range(S)]
  if S >= 3:
    lens[2] = 0
  if S >= 5:
    lens[4] = T - 3
  return logits, lens


class Outputs:
  """What a step wrote, as numpy arrays: state [S, 8], ids [S, max_new], new_count [S], neg_sum [S] float32, events [S, P, 8],
  pieces [P, S, 4]."""

  def __init__(self, state, ids, new_count, neg_sum, events, pieces):
    self.state, self.ids, self.new_count, self.neg_sum, self.events, self.pieces = state, ids, new_count, neg_sum, events, pieces


def drive(step_fn, logits, lens, C, space_id, R, L, M, cuts, sit_out=True, finish_apart=(), extra=3, on_step=None):
  """Feed every stream cuts[s] rows per step (stream s sits every fourth step out) until its length is consumed; the step that brings
  the last rows finishes it -- or, for the streams in ``finish_apart``, a later step without rows -- and offers up to ``extra`` rows
  past the limit.  ``step_fn(buf [n, 32], rows [n, 2], table [S, 4], max_rows, P) -> Outputs``.  Every step is compared with the
  specification.  Returns the number of events and situations seen, per stream the finals
  [dict(event=[8 words], ids=[...])] and the streams' specifications."""
  S = len(lens)
  specs = [EO.Spec(logits[s], C, space_id, R, L, M, lens[s]) for s in range(S)]
  max_rows = max(cuts) + extra
  P = EO.pieces_needed(max_rows, R, L, M)
  fed, started, done, pending_finish = [0] * S, [False] * S, [False] * S, [False] * S
  seen, k = {1: 0, 2: 0, 3: 0, 4: 0}, 0
  seen.update({name: 0 for name in SITUATIONS})
  finals, open_ids = [[] for _ in range(S)], [[] for _ in range(S)]
  while not all(done):
    table = np.zeros((S, 4), np.int32)
    table[:, 2] = -1
    rows, chunks, plan = [], [], {}
    for s in range(S):
      if done[s] or (sit_out and not pending_finish[s] and (k + s) % 4 == 3):
        continue
      n = 0 if pending_finish[s] else min(cuts[s], lens[s] - fed[s])
      finishing = pending_finish[s] or (fed[s] + n >= lens[s] and s not in finish_apart)
      if fed[s] + n >= lens[s] and not finishing:
        pending_finish[s] = True
      offered = n + (min(extra, len(logits[s]) - fed[s] - n) if finishing else 0)
      table[s] = (len(rows) if offered else 0, offered, lens[s] if finishing else -1, 0 if started[s] else 1)
      rows += [(s, fed[s] + j) for j in range(offered)]
      chunks.append(logits[s][fed[s]:fed[s] + offered])
      plan[s] = (fed[s], fed[s] + n, int(table[s, 0]), not started[s], finishing)
      fed[s] += n
      started[s] = True
      done[s] = finishing
    buf = np.full((max(len(rows), 1), PITCH), POISON, np.float32)
    if rows:
      buf[:len(rows), :C] = np.concatenate(chunks)
    out = step_fn(buf, np.asarray(rows if rows else [(0, 0)], np.int32), table, max_rows, P)
    for s in range(S):
      if s not in plan:
        if started[s]:                                              # sitting out: nothing new, the record as it was
          assert out.new_count[s] == 0 and out.events[s, 0, 0] == 0 and (out.pieces[:, s] == EO.UNUSED).all(), (k, s)
          assert tuple(out.state[s]) == specs[s].state(fed[s], done[s])[0], (k, s)
        continue
      a, b, first_row, reset, finishing = plan[s]
      want = specs[s].step(a, b, first_row, reset, finishing, P)
      got_events = []
      for e in out.events[s]:
        if e[0] == 0:
          break
        got_events.append(e.tolist())
      where = (k, s, a, b, finishing)
      assert got_events == want['events'], (where, got_events, want['events'])
      assert [tuple(p) for p in out.pieces[:, s].tolist()] == want['pieces'], (where, out.pieces[:, s].tolist(), want['pieces'])
      assert out.new_count[s] == len(want['ids']) and out.ids[s, :len(want['ids'])].tolist() == want['ids'], (where, want['ids'])
      assert tuple(out.state[s].tolist()) == want['state'], (where, out.state[s].tolist(), want['state'])
      assert np.float32(out.neg_sum[s]).tobytes() == want['neg_sum'].tobytes(), (where, out.neg_sum[s], want['neg_sum'])
      prev = 0
      for e in got_events:                                          # a stretch's ids: what earlier steps brought plus this step's up to ids_end
        seen[e[0]] += 1
        open_ids[s] += out.ids[s, prev:e[5]].tolist()
        prev = e[5]
        if e[0] in EO.FINAL_KINDS:
          finals[s].append(dict(event=e, ids=open_ids[s]))
        open_ids[s] = []
      open_ids[s] += out.ids[s, prev:out.new_count[s]].tolist()
      # which of the situations the tests must meet this step was
      row_ends = [e[2] for e in specs[s].row_events if a < e[2] <= b]
      seen['first_row'] += a + 1 in row_ends
      seen['last_row'] += b > a and b in row_ends
      seen['two_events'] += len(row_ends) >= 2
      if finishing:
        closing = specs[s].events[len(specs[s].row_events):]
        seen['finish_started'] += bool(closing) and closing[0][0] == EO.END
        seen['finish_unstarted'] += bool(closing) and closing[0][0] == EO.DISCARD
        seen['finish_without_rows'] += a == b
        seen['rows_past_limit'] += table[s, 1] > b - a
    if on_step:
      on_step(k, plan, out, table)
    k += 1
    assert k < 4000
  for s in range(S):                                                # ... and over the whole stream: the specification's finals, in order
    assert [f['event'][:5] + f['event'][7:] for f in finals[s]] == [list(e) for e in specs[s].finals()], s
    for f in finals[s]:                                             # ... each with the greedy ids and the sum of its rows alone
      u0, end = f['event'][1:3]
      assert f['ids'] == EO.collapse(specs[s].k[u0:end], C - 1), (s, u0, end)
      assert f['event'][6] == int(specs[s].neg_sum(u0, end).view(np.int32)), (s, u0, end)
  return seen, finals, specs


def host_step_fn(lib, C, space_id, R, L, M, S, guard=7):
  """`step_fn` on st_stream_endpoint_host.  State and outputs start as a pattern; the words behind ids, events and pieces are guards."""
  state = np.full((S, 8), 0x5A5A5A5A, np.int32)
  score = np.full(S * 256, 1e30, np.float32)
  p = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)

  def step(buf, rows, table, max_rows, P):
    ids = np.full(S * max_rows + guard, -77, np.int32)
    events = np.full(S * P * 8 + guard, -77, np.int32)
    pieces = np.full(P * S * 4 + guard, -77, np.int32)
    new_count, neg_sum = np.full(S, -77, np.int32), np.full(S, np.nan, np.float32)
    rc = lib.st_stream_endpoint_host(p(buf), PITCH, C, p(rows), p(table), S, space_id, R, L, M, max_rows, p(state), p(score), p(ids), max_rows,
                                     p(new_count), p(neg_sum), p(events), p(pieces), P)
    assert rc == 0, lib.st_last_error().decode()
    assert (ids[S * max_rows:] == -77).all() and (events[S * P * 8:] == -77).all() and (pieces[P * S * 4:] == -77).all()
    return Outputs(state.copy(), ids[:S * max_rows].reshape(S, max_rows), new_count, neg_sum, events[:S * P * 8].reshape(S, P, 8),
                   pieces[:P * S * 4].reshape(P, S, 4))

  return step


def cut_plans(S):
  """Ways of cutting S streams' rows into steps: every stream with the same cut, and the cuts dealt round the streams."""
  plans = [[c] * S for c in CUTS]
  plans += [[CUTS[(s + shift) % len(CUTS)] for s in range(S)] for shift in (0, 2)]
  return plans


def sweep():
  """(seed, S, C, space_id, R, L, M) of the host sweep: every parameter triple at every class count, space set and not."""
  out = []
  for i, ((R, L, M), C) in enumerate(itertools.product(PARAMS, CLASSES)):
    for space_id in ((C - 2, -1) if C > 2 else (-1,)):
      out.append((i, (1, 3, 5)[i % 3], C, space_id, R, L, M))
  return out


# ---- the recogniser's case (tests/test_gpu_endpoint.py part 3; vetted on float64 logits by tests/test_endpoint_cpu.py) -------------

RECOGNIZER_SECONDS = dict(silence=0.16, lead=0.4, max_utterance=0.8)       # R, L, M = 8, 20, 40 rows of 20 ms
BLANK_BIAS = 6.02            # added to the blank's last-layer bias: 0.4 above the best label where the input is silent
SPEECH_AMPLITUDE = 4.0
RECOGNIZER_PLANS = {         # (frames, amplitude) stretches of the two feature streams: silence is zeros, speech is noise
    'a': (5, [(300, 0.0), (120, SPEECH_AMPLITUDE), (260, 0.0), (160, SPEECH_AMPLITUDE), (240, 0.0), (400, SPEECH_AMPLITUDE), (200, 0.0),
              (100, SPEECH_AMPLITUDE)]),
    'b': (6, [(150, SPEECH_AMPLITUDE), (300, 0.0), (330, SPEECH_AMPLITUDE), (220, 0.0), (101, SPEECH_AMPLITUDE)]),
}


def recognizer_model():
  """The tiny model of tests/test_gpu_lm_beam.py with the blank's bias raised: (layers, params)."""
  from tests import workloads as WL
  layers = WL.w2l_layers(16, width=40, fc=72)
  params = WL.xavier_params(layers, seed=21, bias_range=0.3)
  F, b = params[-1][0] * 12.0, params[-1][1] * 4.0
  b[28] += BLANK_BIAS
  params[-1] = (F, b)
  return layers, params


def recognizer_features(name):
  seed, plan = RECOGNIZER_PLANS[name]
  rng = np.random.default_rng(seed)
  return np.concatenate([rng.standard_normal((n, 16)) * a for n, a in plan]).astype(np.float32)
