"""Keyword spotting in live streams on the GPU: st_ctc_spot_stream_step against its host form (st_ctc_spot_stream_host -- the two
share their arithmetic, csrc/ctc_spot_core.h and csrc/ctc_spot_stream_core.h) BIT FOR BIT on every step's events and counts and on
the state the step leaves, however the rows are cut and with the other streams of the launch interleaved, idle, resetting or
finishing; both packings; the device's own offline trace; guard words, poison in the pitch columns, single -inf logits; refusals
without a launch.  Then the whole path: `StreamingRecognizer(spot=...)` alone, with a beam search, with endpointing and with both,
and `speecht-cli stream --keyword`."""
import os

import numpy as np
import pytest

from tests import spot_stream_cases as SC
from tests import spot_stream_oracle as SO
from tests import workloads as WL

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

NEG_INF = float('-inf')
LONG = [(7 * i + 3) % 28 for i in range(100)]                              # 201 states: four per lane
SETS = {
    'fill': [[1] * 31],                                                    # one wave of 63 states
    'spill': [[1] * 31, [2]],
    'kpl2': [[(3 * i) % 4 for i in range(32)]],
    'ones': [[k % 4] for k in range(21)],
    'aa': [[0, 0]],
    'mixed': [[2, 0, 3], [0], [1, 1], [3, 1, 0, 2, 2, 0, 3]],
    'long': [LONG, [2, 0], [3]],
}


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def _streams(C, keywords, lengths, seed):
  """Noise over the classes the keywords use, with tight readings of the keywords planted where they fit, and single -inf logits."""
  out = {}
  for s, T in enumerate(lengths):
    x = SC.noise(T, C, seed + s, scale=1.5)
    at = 3 + s
    for n, k in enumerate(keywords):
      k = [i % (C - 1) for i in k]
      stay = 1 + (n + s) % 2
      if at + stay * len(k) + sum(p == q for p, q in zip(k, k[1:])) + 2 < T:
        at = SC.plant(x, at, k, C - 1, stay=stay) + n % 3
    x[5 % T, 0] = -np.inf
    x[(T - 2) % T, C - 1] = -np.inf
    out[s] = x
  return out


def _pair(keywords, C, S, threshold, hold, dev, pack=1, max_events=64):
  return (SC.Runner(keywords, C, S, threshold, hold, pack=pack, max_events=max_events),
          SC.Runner(keywords, C, S, threshold, hold, pack=pack, max_events=max_events, device=dev))


def _same_step(host, device, feeds):
  """One step through both runners: equal events, counts and state."""
  frames = host.frames.copy()
  want = host.step(feeds)
  device.frames[:] = frames
  got = device.step(feeds)
  assert got == want
  hs, ds = host.state_words(), device.state_words()
  per = host.state_bytes // 4
  for s in range(host.S):                                                  # (a stream never reset holds each runner's own garbage)
    if s in host.started:
      assert np.array_equal(hs[s * per:(s + 1) * per], ds[s * per:(s + 1) * per]), s
  return want


def _schedule(host, device, streams, sizes, plan):
  """Feed the streams side by side: stream s takes its next sizes[(i + s) % len] rows in step i unless ``plan(i, s)`` says 'idle';
  'reset' starts it again from its first row.  Every stream finishes in the step after its last row.  -> {s: all events since its
  last reset}."""
  at = {s: 0 for s in streams}
  done, got = set(), {s: set() for s in streams}
  host.started = device.started = set()
  i = 0
  while len(done) < len(streams):
    feeds = {}
    for s, x in streams.items():
      if s in done:
        continue
      what = plan(i, s)
      if what == 'idle' and s in host.started:
        continue
      reset = s not in host.started or what == 'reset'
      if reset:
        at[s], got[s] = 0, set()
      n = min(sizes[(i + s) % len(sizes)], len(x) - at[s])
      finish = at[s] == len(x)
      feeds[s] = (x[at[s]:at[s] + n], len(x) if finish else -1, reset)
      host.started.add(s)
      at[s] += n
      if finish:
        done.add(s)
    for s, (ev, count) in _same_step(host, device, feeds).items():
      assert count == len(ev)
      if s in got:
        got[s] |= ev
    i += 1
  return got


@pytest.mark.parametrize('name,C', [('fill', 5), ('spill', 5), ('kpl2', 5), ('ones', 5), ('aa', 5), ('mixed', 5), ('long', 29), ('mixed', 29)])
def test_kernel_equals_host_form_however_the_rows_are_cut(dev, name, C):
  keywords = SETS[name]
  streams = _streams(C, keywords, (150, 97, 40), 31)
  plans = [lambda i, s: None,
           lambda i, s: 'idle' if (i + s) % 3 == 0 else ('reset' if (i, s) == (4, 1) else None)]
  seen = []
  for sizes, plan, threshold, hold in (([70, 1, 63, 2], plans[0], NEG_INF, 2), ([64, 65, 5], plans[1], -0.69, 3), ([9], plans[0], NEG_INF, 2)):
    host, device = _pair(keywords, C, 3, threshold, hold, dev, max_events=2048)
    got = _schedule(host, device, streams, sizes, plan)
    for s, x in streams.items():
      assert got[s] == SO.as_set(e[:5] for e in SO.stream_events(x, [[i % (C - 1) for i in k] for k in keywords], threshold, hold)), s
    seen.append(got)
  assert seen[0] == seen[2] and any(seen[0].values())


@pytest.mark.parametrize('name,C', [('mixed', 29), ('long', 29), ('ones', 5)])
def test_both_packings_and_the_offline_trace(dev, name, C):
  from tests.test_gpu_spot import device_spot
  keywords = [[i % (C - 1) for i in k] for k in SETS[name]]
  streams = _streams(C, keywords, (120, 64, 65), 77)
  got = {}
  for pack in (0, 1):
    host, device = _pair(keywords, C, 3, NEG_INF, 2, dev, pack=pack, max_events=2048)
    got[pack] = _schedule(host, device, streams, [10, 33], lambda i, s: None)
    assert device.n_waves == (len(keywords) if pack == 0 else {'mixed': 1, 'long': 1, 'ones': 1}[name])
  assert got[0] == got[1] and all(got[1].values())
  T = max(len(x) for x in streams.values())
  dense = np.zeros((3, T, C), np.float32)
  for s, x in streams.items():
    dense[s, :len(x)] = x
  jobs = [(s, k) for s in range(3) for k in range(len(keywords))]
  _, _, status, trv, trs = device_spot(dev, dense, [len(streams[s]) for s in range(3)], keywords, jobs)
  assert not np.asarray(status).any()
  for s in range(3):
    for k, a, e, kind, bits in got[1][s]:
      j = s * len(keywords) + k
      assert np.float64(trv[j][e - 1]).view(np.int64) == bits and trs[j][e - 1] == a, (s, k, a, e)


def test_overflow_keeps_the_true_count_and_the_buffer(dev):
  C, keywords = 5, SETS['mixed']
  streams = _streams(C, keywords, (90, 60), 5)
  host, device = _pair(keywords, C, 2, NEG_INF, 1, dev, max_events=2)
  host.started = device.started = {0, 1}
  before = device.d_events.cpu().numpy().copy()
  want = host.step({0: (streams[0], -1, True), 1: (streams[1][:3], -1, True)})
  device.frames[:] = 0
  got = device.step({0: (streams[0], -1, True), 1: (streams[1][:3], -1, True)})
  all0 = SO.as_set(e[:5] for e in SO.stream_events(streams[0], keywords, NEG_INF, 1, finish=False))
  assert got[0][1] == want[0][1] == len(all0) > 2 and len(got[0][0]) == 2 and got[0][0] <= all0
  all1 = SO.as_set(e[:5] for e in SO.stream_events(streams[1][:3], keywords, NEG_INF, 1, finish=False))
  assert got[1][1] == want[1][1] == len(all1) and got[1][0] <= all1 and len(got[1][0]) == min(len(all1), 2)
  used = min(len(all1), 2)
  after = device.d_events.cpu().numpy()[16:-16].reshape(2, 2, 8)
  assert np.array_equal(after[1, used:], before[16:-16].reshape(2, 2, 8)[1, used:])               # unused slots keep their garbage


def test_validation_returns_an_error_without_a_launch(dev):
  from speecht_amd._lib import launch_trace
  C, keywords = 5, SETS['mixed']
  x = SC.noise(6, C, 1)
  device = SC.Runner(keywords, C, 1, -0.69, 2, device=dev)
  unbound = SC.Runner(keywords, C, 1, -0.69, 2, device=dev)
  unbound.plan[8:10] = 0                                                   # a plan without a device copy
  state = device.d_state.clone()
  with launch_trace() as tr:
    device.step({0: (x, -1, True)}, threshold=float('nan'), want=-1)
    device.step({0: (x, -1, True)}, threshold=1e-9, want=-1)
    device.step({0: (x, -1, True)}, hold=0, want=-1)
    unbound.step({0: (x, -1, True)}, want=-1)
    device.C = 6
    device.step({0: (SC.noise(6, 6, 1), -1, True)}, want=-1)
    device.C = 5
    good = device.plan.copy()
    device.plan[0] ^= 0x100
    device.step({0: (x, -1, True)}, want=-1)
    device.plan[:] = good
  assert tr.lines == [] and torch.equal(state, device.d_state)
  # a device copy that is no plan: the kernel does nothing (the counts are cleared, the state keeps its bits)
  device.d_plan[0] += 1
  torch.cuda.synchronize()
  assert device.step({0: (x, -1, True)})[0] == (set(), 0) and torch.equal(state, device.d_state)


# ---- the whole path ------------------------------------------------------------------------------------------------------------

SMALL = WL.w2l_layers(16, width=24, fc=40)
WATCH = ['a', 'th', 'e ', 'cat']


@pytest.fixture(scope='module')
def small(dev):
  from speecht_amd.engine import Wav2LetterEngine
  params = WL.xavier_params(SMALL, seed=7)
  params[-1] = (params[-1][0] * 12.0, params[-1][1] * 4.0)        # (peakier posteriors, as the other stream tests use)
  eng = Wav2LetterEngine(SMALL, device=dev)
  eng.set_weights(params)
  return eng


def _spotter(max_events=512):
  from speecht_amd.streaming import StreamSpotter
  return StreamSpotter(WATCH, threshold=NEG_INF, hold=0.1, max_events=max_events)


def _solo(eng, x, chunk, spot=None, beam=None, endpoint=None):
  """One stream alone -> (hits as tuples, hits per step, everything else the steps reported, the logits, the recogniser)."""
  from speecht_amd.streaming import StreamingRecognizer
  rec = StreamingRecognizer(eng, 2, max_chunk_frames=64, beam=beam, endpoint=endpoint, spot=spot)
  rec.open()
  slot = rec.open()                                               # (slot 1: slot 0 stays idle beside it)
  hits, rest, rows = [], [], []
  for at in list(range(0, len(x), chunk)) + ['end']:
    r = rec.finish(slot, return_logits=True) if at == 'end' else rec.step({slot: x[at:at + chunk]}, return_logits=True)
    rows.append(r.logits[slot])
    rest.append((at, r.ids[slot], r.score[slot], r.hyp.get(slot), r.stable.get(slot), r.logp.get(slot), repr(r.finals.get(slot)),
                 r.open_ids.get(slot)))
    if spot is not None:
      assert r.hits_lost[slot] == 0 and r.hits[slot] == sorted(r.hits[slot], key=lambda h: (h.end_frame, h.index))
      hits += [(h.index, h.start_frame, h.end_frame, int(h.flushed), int(np.float64(h.score).view(np.int64))) for h in r.hits[slot]]
    else:
      assert r.hits == {} and r.hits_lost == {}
  return hits, rest, np.concatenate(rows), rec


def _decoders(which):
  from speecht_amd.streaming import Endpointing, StreamBeam
  beam = (lambda: StreamBeam(beam_width=16, max_seconds=4.0)) if 'beam' in which else (lambda: None)
  endpoint = (lambda: Endpointing(silence=0.06, lead=0.2, max_utterance=0.6)) if 'endpoint' in which else (lambda: None)
  return beam, endpoint


@pytest.mark.parametrize('which', ['alone', 'beam', 'endpoint', 'beam+endpoint'])
def test_whole_path_two_chunkings_equal_the_host_form(dev, small, which):
  beam, endpoint = _decoders(which)
  x = WL.synthetic_features(151, 151, 16).astype(np.float32)
  a, rest_a, logits, rec_a = _solo(small, x, 50, _spotter(), beam(), endpoint())
  b, rest_b, logits_b, _ = _solo(small, x, 25, _spotter(), beam(), endpoint())
  _, rest_plain, logits_plain, rec_plain = _solo(small, x, 50, None, beam(), endpoint())
  assert np.array_equal(logits, logits_b) and np.array_equal(logits, logits_plain)
  assert sorted(a) == sorted(b) and len(a) == len(set(a)) > 0
  # the hits are the host form's on the stream's own rows (the rows past the decode limit are not consumed)
  spot = _spotter()
  host = SC.Runner(spot.ids, 29, 1, spot.threshold, spot.frames(2), max_events=512)
  assert host.hold == 5
  want, count = host.step({0: (logits, 151 // 2, True)})[0]
  assert set(a) == want and count == len(a) and any(kind == 1 for _, _, _, kind, _ in a)
  # the decoders report what they report without a spotter; two launches come on top (the memset of the counts, the lattices)
  assert rest_a == rest_plain and rec_a.launches == rec_plain.launches + 2
  assert not hasattr(rec_plain, 'spot_state') and rec_plain._spot is None


def test_streams_side_by_side_lost_hits_and_reopened_slots(dev, small):
  from speecht_amd.streaming import StreamError, StreamingRecognizer
  x = WL.synthetic_features(31, 140, 16).astype(np.float32)
  y = WL.synthetic_features(32, 130, 16).astype(np.float32)
  solo_x, solo_y = sorted(_solo(small, x, 40, _spotter())[0]), sorted(_solo(small, y, 40, _spotter())[0])
  tup = lambda hits: [(h.index, h.start_frame, h.end_frame, int(h.flushed), int(np.float64(h.score).view(np.int64))) for h in hits]
  rec = StreamingRecognizer(small, 2, max_chunk_frames=64, spot=_spotter())
  with pytest.raises(StreamError, match='spotter'):
    rec.step({}, fetch=False)
  a, b = rec.open(), rec.open()
  r = rec.step({a: y[:110], b: x[:40]})
  got_x, got_y = tup(r.hits[b]), []
  rec.close(a)                                                    # a's stream is dropped mid-way; its slot starts clean for y
  a2 = rec.open()
  assert a2 == a
  for k in range(1, 4):
    feeds = {a2: y[40 * (k - 1):40 * k]}
    if k < 3:
      feeds[b] = x[40 * k:40 * (k + 1)]
    r = rec.step(feeds)
    got_y += tup(r.hits[a2])
    got_x += tup(r.hits.get(b, []))
  r = rec.step({a2: y[120:], b: x[120:]})
  got_y += tup(r.hits[a2])
  got_x += tup(r.hits[b])
  r = rec.finish_many([a2, b])
  got_y += tup(r.hits[a2])
  got_x += tup(r.hits[b])
  assert sorted(got_y) == solo_y and sorted(got_x) == solo_x and solo_x and solo_y
  # a buffer of one event per step: the rest is counted, never silent
  rec = StreamingRecognizer(small, 1, max_chunk_frames=64, spot=_spotter(max_events=1))
  s = rec.open()
  r = rec.step({s: x})
  assert len(r.hits[s]) <= 2 and r.hits_lost[s] > 0               # (140 frames are three passes of up to 64)
  ref = StreamingRecognizer(small, 1, max_chunk_frames=64, spot=_spotter())
  t = ref.open()
  q = ref.step({t: x})
  assert q.hits_lost[t] == 0 and len(r.hits[s]) + r.hits_lost[s] == len(q.hits[t]) and set(tup(r.hits[s])) <= set(tup(q.hits[t]))


def test_cli_stream_with_keywords(dev, golden_dir, tmp_path, capsys, monkeypatch):
  import importlib.machinery
  import importlib.util
  from speecht_amd import transcription
  from speecht_amd.speech_input import SingleInputLoader
  from speecht_amd.speech_model import Session, Wav2LetterModel
  from speecht_amd.streaming import StreamSpotter, hit_line, stream_audio
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  loader = importlib.machinery.SourceFileLoader('speecht_cli_stream_spot_gpu', os.path.join(root, 'speecht-cli'))
  spec = importlib.util.spec_from_loader('speecht_cli_stream_spot_gpu', loader)
  cli = importlib.util.module_from_spec(spec)
  loader.exec_module(cli)
  flac = os.path.join(golden_dir, '1089-134686-0037.flac')
  samples, rate = transcription.load_native(flac)
  per = int(rate * 200 / 1000.0)
  pieces = [samples[at:at + per] for at in range(0, len(samples), per)]
  model = Wav2LetterModel(SingleInputLoader(128), 128, 29)       # a checkpoint written the way test_gpu_stream.py does
  model.add_training_ops()
  model.add_decoding_ops()
  model.finalize(str(tmp_path / 'log'), 'r', 'record')
  model.init_seed = 1234
  train = tmp_path / 'train'
  (train / 'run').mkdir(parents=True)
  kwfile = tmp_path / 'kw.txt'
  kwfile.write_text('# two of them\nthe\na\n')
  want = []
  with Session(dev) as sess:
    model.init_session(sess)
    model.saver.save(sess, str(train / 'run' / 'speechT'), global_step=model.global_step)
    spot = StreamSpotter(['the', 'a', 'e'], threshold=-5.0, hold=0.2)
    stream_audio(model.engine, pieces, rate, 128, 'running', None, max_piece=per, spot=spot, on_hit=lambda h: want.append(hit_line(h, rate)))
  cwd = tmp_path / 'cwd'
  cwd.mkdir()
  monkeypatch.chdir(cwd)
  capsys.readouterr()
  code = cli.main(['stream', '--train-dir', str(train), '--run-name', 'run', '--device', dev, '--keywords', str(kwfile), '--keyword', 'e',
                   '--spot-threshold', '-5.0', '--spot-hold', '0.2', flac])
  lines = capsys.readouterr().out.splitlines()
  assert code == 0 and lines[-1].startswith(flac + '\t')
  hits = [l for l in lines[:-1] if len(l.split('\t')) == 5]
  assert hits == want and len(hits) > 0
  seconds = len(samples) / float(rate)
  for start, end, keyword, score, per_frame in (l.split('\t') for l in hits):
    assert 0.0 <= float(start) < float(end) <= seconds + 0.04 and keyword in ('the', 'a', 'e')
    assert float(score) <= 0.0 and -5.0001 <= float(per_frame) <= 0.0
  assert sorted(os.listdir(str(cwd))) == []
