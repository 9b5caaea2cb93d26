"""Hotword biasing: phrases the beam searches should favour (a contact list, product names, the vocabulary of a meeting).

A hypothesis with prefix x scores, during either CTC beam search, ``weight * (M(x) + r(x))`` on top of its CTC mass and LM terms: M
is the number of characters of completed phrase occurrences banked so far, r the length of the partial match still open -- a partial
match earns credit while it grows and gives it back when it fails.  At the end of the utterance the open match is resolved: the
phrases it completed are banked, the rest is forfeited.  The rules, on strings, are the specification in tests/hotword_oracle.py
(also include/speecht_hip.h); they are pure functions of (trie node, label), so this module tabulates them once per phrase set --

  next int32 [N][32], gain float32 [N][32] = weight * (banked + depth(next) - depth(n)), fin float32 [N] = weight * (flush bank - depth(n))

with the trie's nodes numbered breadth first (children by label, the root 0; columns >= 28: the state itself and 0) -- and the
kernels read the tables (`engine.beam_search_decode_nbest(..., hotwords=)`, `engine.lm_beam_search_decode_nbest(..., hotwords=)`).

Matching is by characters anywhere in the text: "cat" is also matched inside "catalog" (give " cat " with its spaces to ask for the
word), and every phrase has the same weight per character.
"""
import numpy as np

from . import vocabulary

LABELS = vocabulary.SIZE          # 28: a-z, apostrophe, space
PITCH = 32                        # columns of a table row
MAX_PHRASE_IDS = 64
MAX_PHRASES = 4096
MAX_STATES = 1 << 20              # st_bias_tables.n_states


class HotwordError(ValueError):
  """A phrase list that cannot be used."""


def phrase_ids(phrase):
  """Ids of a phrase given as text (lower-cased; letters, apostrophe, space) or as a list of ids 0..27; raises HotwordError for an
  empty one, one of more than MAX_PHRASE_IDS ids or one with a character outside the vocabulary."""
  if isinstance(phrase, str):
    text = phrase.lower()
    ids = vocabulary.sentence_to_ids(text)
    bad = sorted({ch for ch, i in zip(text, ids) if not 0 <= i < LABELS})
    if bad:
      raise HotwordError('hotword {!r} has characters outside the vocabulary: {}'.format(text, ' '.join(map(repr, bad))))
  else:
    ids = [int(i) for i in phrase]
    if any(not 0 <= i < LABELS for i in ids):
      raise HotwordError('hotword ids must lie in 0..{}, got {}'.format(LABELS - 1, ids))
  if not ids:
    raise HotwordError('hotword is empty')
  if len(ids) > MAX_PHRASE_IDS:
    raise HotwordError('hotword of {} characters is too long (at most {})'.format(len(ids), MAX_PHRASE_IDS))
  return ids


class Hotwords:
  """``Hotwords(phrases, weight=1.0)``: phrases are strings or id lists (duplicates dropped, at most MAX_PHRASES); ``weight`` >= 0 is
  the credit per matched character, in the units of the search's scores -- natural log for a search on logits, log10 for
  ``input_transform='log10_softmax'``.  The default 1.0 is a guess: nobody has tuned it on data.  An empty list is allowed and biases
  nothing."""

  def __init__(self, phrases, weight=1.0):
    weight = float(weight)
    if not (weight >= 0.0 and np.isfinite(weight)):
      raise HotwordError('hotword weight must be finite and >= 0, got {}'.format(weight))
    if isinstance(phrases, str):
      raise HotwordError('hotwords: give a list of phrases, not one string')
    seen, unique = set(), []
    for p in phrases:
      ids = tuple(phrase_ids(p))
      if ids not in seen:
        seen.add(ids)
        unique.append(ids)
    if len(unique) > MAX_PHRASES:
      raise HotwordError('{} hotwords given, at most {}'.format(len(unique), MAX_PHRASES))
    self.phrases, self.weight = unique, weight
    self._build()
    self._device = {}

  def __len__(self):
    return len(self.phrases)

  def _build(self):
    # the trie, then its nodes renumbered breadth first with children in label order
    kids, ends = [{}], [False]
    for p in self.phrases:
      n = 0
      for c in p:
        m = kids[n].get(c)
        if m is None:
          m = kids[n][c] = len(kids)
          kids.append({})
          ends.append(False)
        n = m
      ends[n] = True
    order, parent, label, depth = [0], [0], [-1], [0]
    for i in range(len(kids)):                      # `order` grows while it is read: a queue
      if i >= len(order):
        break
      for c in sorted(kids[order[i]]):
        order.append(kids[order[i]][c])
        parent.append(i)
        label.append(c)
        depth.append(depth[i] + 1)
    n_states = len(order)
    if n_states > MAX_STATES:
      raise HotwordError('hotwords: {} trie nodes, at most {}'.format(n_states, MAX_STATES))
    new_of = {old: new for new, old in enumerate(order)}
    child = np.full((n_states, LABELS), -1, np.int64)
    end = np.zeros(n_states, bool)
    for new, old in enumerate(order):
      end[new] = ends[old]
      for c, k in kids[old].items():
        child[new, c] = new_of[k]
    has_kids = (child >= 0).any(axis=1)
    depth = np.array(depth, np.int64)
    # by depth: a failed match restarts on a strictly shorter string, so the rows it needs are complete
    nxt = np.zeros((n_states, LABELS), np.int64)
    bank = np.zeros((n_states, LABELS), np.int64)
    flush = np.zeros(n_states, np.int64)
    longest = np.zeros(n_states, np.int64)          # depth of the deepest phrase end on the node's path, itself included
    for n in range(n_states):
      if n == 0:
        row_next, row_bank = np.zeros(LABELS, np.int64), np.zeros(LABELS, np.int64)
      else:
        longest[n] = depth[n] if end[n] else longest[parent[n]]
        path, m = [], n
        while m:
          path.append(label[m])
          m = parent[m]
        path.reverse()
        s, banked = 0, int(longest[n])
        for c in path[max(int(longest[n]), 1):]:    # u: the path without the banked phrase, or without its first character
          banked += int(bank[s, c])
          s = int(nxt[s, c])
        row_next, row_bank = nxt[s].copy(), banked + bank[s]
        flush[n] = banked + flush[s]
      for c in np.flatnonzero(child[n] >= 0):
        k = child[n, c]
        leaf = end[k] and not has_kids[k]
        row_next[c], row_bank[c] = (0, depth[k]) if leaf else (k, 0)
      nxt[n], bank[n] = row_next, row_bank
    self.n_states = n_states
    self._depth, self._bank, self._flush = depth, bank, flush
    self.next = np.tile(np.arange(n_states, dtype=np.int32)[:, None], (1, PITCH))
    self.next[:, :LABELS] = nxt
    self.gain = np.zeros((n_states, PITCH), np.float32)
    self.gain[:, :LABELS] = self.weight * (bank + depth[nxt] - depth[:, None]).astype(np.float64)
    self.fin = (self.weight * (flush - depth).astype(np.float64)).astype(np.float32)

  def score(self, ids):
    """-> (during, final) in float64: the bias the prefix ``ids`` carries during the search, weight * (M + r), and at the end of the
    utterance, weight * (M + what the flush banks).  Ids outside 0..27 neither advance nor break a match."""
    n, m = 0, 0
    for c in ids:
      c = int(c)
      if 0 <= c < LABELS:
        m += int(self._bank[n, c])
        n = int(self.next[n, c])
    return self.weight * (m + int(self._depth[n])), self.weight * (m + int(self._flush[n]))

  def device_tables(self, device):
    """(next, gain, fin) as torch tensors on ``device``, uploaded once per device."""
    import torch
    key = str(torch.device(device))
    if key not in self._device:
      self._device[key] = tuple(torch.as_tensor(np.ascontiguousarray(a)).to(device) for a in (self.next, self.gain, self.fin))
    return self._device[key]


class HotwordSets:
  """``HotwordSets(sets)``: several phrase sets (each a `Hotwords`, with a weight of its own, or a list of phrases) in ONE table, for
  searches that run side by side with a set each -- the streams of a `streaming.StreamingRecognizer`.  Set 0 is always the empty set
  (one state, every gain 0: a search rooted there returns the unbiased search's bits); the given sets follow as 1, 2, ...  Set k's
  states are the rows ``base[k] .. base[k + 1]`` of ``next`` / ``gain`` / ``fin``, its ``next`` values shifted by ``base[k]`` -- a
  match that returns to the root returns to row ``base[k]``, set k's own -- so a search that STARTS in state ``base[k]`` never leaves
  set k's rows.  At most MAX_STATES states in all."""

  def __init__(self, sets):
    if isinstance(sets, (str, Hotwords)):
      raise HotwordError('hotword sets: give a list of Hotwords')
    self.sets = [Hotwords([])] + [s if isinstance(s, Hotwords) else Hotwords(s) for s in sets]
    counts = [s.n_states for s in self.sets]
    self.base = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    self.n_states = int(self.base[-1])
    if self.n_states > MAX_STATES:
      raise HotwordError('hotword sets: {} trie nodes in all, at most {}'.format(self.n_states, MAX_STATES))
    self.next = np.concatenate([s.next + np.int32(b) for s, b in zip(self.sets, self.base)])
    self.gain = np.concatenate([s.gain for s in self.sets])
    self.fin = np.concatenate([s.fin for s in self.sets])
    self._device = {}

  def __len__(self):
    return len(self.sets)

  def root(self, index):
    """The state a search of set ``index`` starts in."""
    if not isinstance(index, (int, np.integer)) or not 0 <= index < len(self.sets):
      raise HotwordError('hotword set {!r}: sets 0..{} exist'.format(index, len(self.sets) - 1))
    return int(self.base[index])

  def tables(self, index):
    """Set ``index`` alone, as the whole-utterance searches take it: its `Hotwords`."""
    self.root(index)
    return self.sets[index]

  device_tables = Hotwords.device_tables


def from_flags(flags):
  """The `Hotwords` of ``--hotwords FILE`` / ``--hotword TEXT`` / ``--hotword-weight X``, or None when neither list is given."""
  phrases = []
  if getattr(flags, 'hotwords', None):
    from .spotting import read_keywords
    phrases += read_keywords(flags.hotwords)
  phrases += [p.lower() for p in (getattr(flags, 'hotword', None) or [])]
  if not phrases:
    return None
  return Hotwords(phrases, getattr(flags, 'hotword_weight', 1.0))
