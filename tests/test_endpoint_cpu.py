"""Endpointing without a GPU: properties of the specification (tests/endpoint_oracle.py) on seeded silent / speech patterns, the
`Endpointing` settings and their conversion to frames, the flags of `speecht-cli stream --endpoint`, and the vetting of the case the
GPU test of `StreamingRecognizer(endpoint=...)` runs: on float64 logits it must hold several events of every kind."""
import importlib.machinery
import importlib.util
import os

import numpy as np
import pytest

from tests import endpoint_cases as EC
from tests import endpoint_oracle as EO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _patterns():
  rng = np.random.RandomState(3)
  for R, L, M in EC.PARAMS:
    for density in (0.1, 0.5, 0.9):
      yield R, L, M, rng.rand(rng.randint(0, 150)) < density
    yield R, L, M, np.repeat(rng.rand(12) < 0.5, rng.randint(1, M + 4, 12))      # long runs


def test_events_partition_the_rows_and_respect_the_bounds():
  kinds = {1: 0, 2: 0, 3: 0, 4: 0}
  for R, L, M, silent in _patterns():
    events = EO.segment(silent, R, L, M)
    at, index = 0, 0
    for kind, u0, end, first, last, idx in events:
      assert u0 == at and end > u0 and end - u0 <= M, (R, L, M, u0, end)           # adjacent, non-empty, never longer than M
      at = end
      kinds[kind] += 1
      if kind == EO.DISCARD:
        assert silent[u0:end].all() and (first, last) == (-1, -1) and idx == index
        assert end - u0 == L or end == len(silent)                                # a discard is L rows, or what was left at the end
      else:
        assert u0 <= first <= last < end and not silent[first] and not silent[last] and silent[u0:first].all() and silent[last + 1:end].all()
        assert idx == index and first - u0 < L                                    # (a longer lead would have been dropped first)
        if kind == EO.SILENCE:
          assert end - 1 - last == R
        elif kind == EO.LENGTH:
          assert end - u0 == M and end - 1 - last < R
        else:
          assert end == len(silent) and end - 1 - last < R
        index += 1
    assert at == len(silent)                                                      # finals and discards cover every consumed row
    assert [e for e in events if e[2] < len(silent)] == [e for e in EO.segment(silent, R, L, M, finished=False) if e[2] < len(silent)]
  assert all(n > 50 for n in kinds.values()), kinds


def test_a_prefix_has_the_events_of_the_whole_stream():
  """The rule looks at no later row: the events of the first n rows are those of the whole stream that end at or before n."""
  for R, L, M, silent in _patterns():
    whole = EO.segment(silent, R, L, M, finished=False)
    for n in range(0, len(silent), 7):
      assert EO.segment(silent[:n], R, L, M, finished=False) == [e for e in whole if e[2] <= n]


def test_events_per_step_stay_within_the_piece_formula():
  for R, L, M, silent in _patterns():
    ends = [e[2] for e in EO.segment(silent, R, L, M, finished=False)]
    for n in (1, 2, 7, 10, 83):
      P = EO.pieces_needed(n, R, L, M)
      assert P == 2 + (n - 1) // min(L, R + 1, M)
      for a in range(0, len(silent)):                                             # every window of n rows
        assert sum(1 for e in ends if a < e <= a + n) <= P - 1
  assert EO.pieces_needed(13, 25, 50, 1500) == 2 and EO.pieces_needed(27, 25, 50, 1500) == 3


def test_endpointing_validates_and_converts_seconds_to_frames():
  from speecht_amd.streaming import Endpointing, StreamError
  e = Endpointing()
  assert (e.silence, e.lead, e.max_utterance, e.space_id) == (0.5, 1.0, 30.0, 'auto')
  assert e.frames(2, 29) == (25, 50, 1500, 27) and e.frames(2, 5) == (25, 50, 1500, -1) and e.frames(1, 29) == (50, 100, 3000, 27)
  assert Endpointing(0.05, 0.1, 0.1).frames(2, 29) == (3, 5, 5, 27)               # rounded up; lead == max_utterance is allowed
  assert Endpointing(0.001, 0.001, 0.001).frames(2, 29)[:3] == (1, 1, 1)
  assert Endpointing(space_id=-1).frames(2, 29)[3] == -1 and Endpointing(space_id=3).frames(2, 5)[3] == 3
  assert Endpointing(**EC.RECOGNIZER_SECONDS).frames(2, 29) == (8, 20, 40, 27)
  for bad in (dict(silence=0), dict(silence=-1.0), dict(lead=0), dict(max_utterance=0), dict(silence=float('nan')), dict(lead=float('inf')),
              dict(lead=2.0, max_utterance=1.0), dict(space_id=-2), dict(space_id='space'), dict(space_id=1.5)):
    with pytest.raises(StreamError):
      Endpointing(**bad)
  with pytest.raises(StreamError, match='no class'):
    Endpointing(space_id=29).frames(2, 29)
  assert 'not tuned' in Endpointing.__doc__


def _cli():
  loader = importlib.machinery.SourceFileLoader('speecht_cli_endpoint', os.path.join(ROOT, 'speecht-cli'))
  spec = importlib.util.spec_from_loader('speecht_cli_endpoint', loader)
  cli = importlib.util.module_from_spec(spec)
  loader.exec_module(cli)
  return cli


def test_cli_stream_endpoint_flags():
  from speecht_amd.streaming import endpoint_of
  cli = _cli()
  _, flags = cli.parse(['stream', 'a.flac'])
  assert (flags.endpoint, flags.endpoint_silence, flags.endpoint_lead, flags.max_utterance) == (False, 0.5, 1.0, 30.0)
  assert endpoint_of(flags) is None
  _, flags = cli.parse(['stream', '-', '--endpoint'])
  e = endpoint_of(flags)
  assert flags.endpoint and (e.silence, e.lead, e.max_utterance) == (0.5, 1.0, 30.0)
  _, flags = cli.parse(['stream', '-', '--endpoint', '--endpoint-silence', '0.3', '--endpoint-lead', '2', '--max-utterance', '12.5'])
  e = endpoint_of(flags)
  assert (e.silence, e.lead, e.max_utterance) == (0.3, 2.0, 12.5)
  for bad in (['stream', 'a.flac', '--endpoint-silence', '0.3'], ['stream', 'a.flac', '--max-utterance', '10'],
              ['stream', 'a.flac', '--endpoint', '--endpoint-silence', '0'], ['stream', 'a.flac', '--endpoint', '--endpoint-lead', '40'],
              ['stream', 'a.flac', '--endpoint', '--max-utterance', 'long']):
    with pytest.raises(SystemExit) as err:
      cli.main(bad)
    assert err.value.code == 2


def test_the_recognizer_case_holds_every_event_with_room_to_spare():
  """Float64 logits of the model and features tests/test_gpu_endpoint.py streams (a streamed row is the whole-utterance row): at least
  two silence finals, a length final and a discard are asked for there; here there are more of each, and a perturbation a hundred times
  the device's error changes no count."""
  from oracle import w2l_oracle as O
  layers, params = EC.recognizer_model()
  R, L, M, space = 8, 20, 40, 27
  for name, least in (('a', {1: 3, 2: 3, 3: 5}), ('b', {1: 1, 2: 3, 3: 5, 4: 1})):
    x = EC.recognizer_features(name).astype(np.float64)
    logits = np.asarray(O.wav2letter_forward(x[None], params, layers))
    logits = logits.reshape(-1, logits.shape[-1])[:len(x) // 2]
    counts = []
    for noise in (0.0, 1e-3):
      rng = np.random.default_rng(1)
      events = EO.segment(EO.silent_rows(logits + rng.standard_normal(logits.shape) * noise, 29, space), R, L, M)
      counts.append({k: sum(1 for e in events if e[0] == k) for k in (1, 2, 3, 4)})
    assert counts[0] == counts[1] and all(counts[0][k] >= n for k, n in least.items()), (name, counts)
