"""The host's part of keyword spotting in live streams (speecht_amd/streaming.py): what `StreamSpotter` accepts and refuses, its
seconds -> frames, its plan, how a step's events become sorted `Hit`s and a count of lost ones, and the flags of `speecht-cli
stream`.  Needs no GPU."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from speecht_amd import spotting
from speecht_amd.streaming import Endpointing, Hit, StreamError, StreamSpotter, hit_line, read_hits, spotter_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spotter_arguments():
  s = StreamSpotter(['Cat', 'the cat'])
  assert s.keywords == ['cat', 'the cat'] and s.ids == [spotting.keyword_ids('cat'), spotting.keyword_ids('the cat')]
  assert s.threshold == spotting.DEFAULT_THRESHOLD and s.hold == 0.3 and s.max_events == 64
  assert StreamSpotter(['a'], threshold=float('-inf')).threshold == float('-inf') and StreamSpotter(['a'], threshold=0).threshold == 0.0
  for bad in (dict(keywords=[]), dict(keywords='cat'), dict(keywords=['cat', 'CAT']), dict(keywords=['']), dict(keywords=['c4t']),
              dict(keywords=['a' * 512]), dict(keywords=[3]), dict(keywords=['a'], threshold=0.1), dict(keywords=['a'], threshold=float('nan')),
              dict(keywords=['a'], hold=0), dict(keywords=['a'], hold=float('inf')), dict(keywords=['a'], hold=float('nan')),
              dict(keywords=['a'], max_events=0), dict(keywords=['a'], max_events=2.5), dict(keywords=['a'], max_events=True)):
    with pytest.raises(StreamError, match='spotting'):
      StreamSpotter(**bad)


@pytest.mark.parametrize('hold,stride', [(0.3, 2), (0.01, 2), (0.02, 2), (0.021, 2), (1.0, 2), (0.3, 1), (0.5, 8)])
def test_hold_counts_frames_as_endpointing_does(hold, stride):
  assert StreamSpotter(['a'], hold=hold).frames(stride) == Endpointing(silence=hold).frames(stride, 29)[0] >= 1
  assert StreamSpotter(['a'], hold=0.3).frames(2) == 15


def test_plan_of_a_spotter():
  s = StreamSpotter(['cat', 'a', 'the cat'])
  plan, waves = s.plan(29)
  assert waves == 1 and plan[2] == 3 and plan[3] == 29 and plan[4] == 1 and plan[1] == len(plan)
  assert s.plan(29, pack=0)[1] == 3
  with pytest.raises(StreamError, match='classes'):
    s.plan(33)
  with pytest.raises(StreamError, match='character'):
    s.plan(5)


def _events(rows, max_events):
  ev = np.full((1, max_events, 8), 0x5A5A5A5A, dtype=np.int32)
  for i, (k, a, e, kind, score) in enumerate(rows[:max_events]):
    ev[0, i, :4] = (k, a, e, kind)
    ev[0, i, 4:6] = np.asarray([score], np.float64).view(np.int32)
    ev[0, i, 6:] = 0
  return ev


def test_hits_are_sorted_and_lost_ones_counted():
  keywords = ['cat', 'a', 'hat']
  rows = [(2, 40, 52, 0, -1.5), (0, 10, 30, 0, -0.25), (1, 28, 30, 0, 0.0), (0, 60, 71, 1, -3.0)]
  (hits, lost), = read_hits(keywords, _events(rows, 8), np.asarray([4], np.int32), 8)
  assert lost == 0 and hits == [Hit('cat', 0, 10, 30, -0.25, False), Hit('a', 1, 28, 30, 0.0, False), Hit('hat', 2, 40, 52, -1.5, False),
                                Hit('cat', 0, 60, 71, -3.0, True)]
  assert hits[0].score_per_frame == -0.25 / 20 and 'flushed' in repr(hits[3]) and 'flushed' not in repr(hits[0])
  # more events than the buffer holds: the first max_events are read, the rest is counted -- never silent
  (hits, lost), = read_hits(keywords, _events(rows, 2), np.asarray([7], np.int32), 2)
  assert lost == 5 and [h.index for h in hits] == [0, 2]
  (hits, lost), = read_hits(keywords, _events([], 2), np.asarray([0], np.int32), 2)
  assert hits == [] and lost == 0


def test_hit_line():
  line = hit_line(Hit('the cat', 1, 50, 75, -2.5, False), 16000).split('\t')
  assert line == ['1.000', '1.500', 'the cat', '-2.5000', '-0.1000']


def test_spotter_of_flags(tmp_path):
  assert spotter_of(types.SimpleNamespace()) is None
  path = tmp_path / 'kw.txt'
  path.write_text('# watch\nthe cat\n\nHat\n')
  s = spotter_of(types.SimpleNamespace(keywords=str(path), keyword=['hat', 'Dog'], spot_threshold=-1.0, spot_hold=0.5))
  assert s.keywords == ['the cat', 'hat', 'dog'] and s.threshold == -1.0 and s.hold == 0.5
  s = spotter_of(types.SimpleNamespace(keyword=['dog']))
  assert s.keywords == ['dog'] and s.threshold == spotting.DEFAULT_THRESHOLD and s.hold == 0.3
  with pytest.raises(StreamError):
    spotter_of(types.SimpleNamespace(keyword=['d0g']))


def _cli(*args):
  return subprocess.run([sys.executable, os.path.join(ROOT, 'speecht-cli'), 'stream'] + list(args), capture_output=True, text=True, timeout=120)


def test_cli_flags(tmp_path):
  r = _cli('--help')
  assert r.returncode == 0 and all(f in r.stdout for f in ('--keywords', '--keyword', '--spot-threshold', '--spot-hold'))
  for args, text in ((['--spot-hold', '0.5', 'x.wav'], 'apply with --keywords or --keyword only'),
                     (['--spot-threshold', '-1', 'x.wav'], 'apply with --keywords or --keyword only'),
                     (['--keyword', 'c4t', 'x.wav'], 'outside the vocabulary'),
                     (['--keyword', 'cat', '--spot-threshold', '0.5', 'x.wav'], 'threshold must be <= 0'),
                     (['--keyword', 'cat', '--spot-hold', '0', 'x.wav'], 'hold must be a positive'),
                     (['--keywords', str(tmp_path / 'none.txt'), 'x.wav'], 'cannot read --keywords')):
    r = _cli(*args)
    assert r.returncode == 2 and text in r.stderr, (args, r.stderr)
