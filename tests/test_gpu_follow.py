"""Following a known script in live streams on the GPU: st_ctc_follow_stream_step against its host form (st_ctc_follow_stream_host:
plain loops over the whole lattice, no tiles) bit for bit -- the cursor trace, the events, the result record and the state -- at the
edges of the state blocks, on planted rows that climb two states per frame into the third block and on random rows, for runs of
exactly 64 rows and a step of 130 rows the entry point cuts into three, three streams in one launch; the overflow of the event
buffer; and `StreamingRecognizer(follow=...)` on the small model: the same however the audio is cut, beside the beam search,
endpointing and the spotter, whose results it leaves alone, and not there at all with follow=None."""
import numpy as np
import pytest

from tests import align_oracle as AO
from tests import follow_oracle as FO
from tests import workloads as WL
from tests.follow_util import Driver

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
C, SPACE = 29, 27


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def _script(rng, L):
  return FO.script_without_repeats(rng, L, C, SPACE) if L > 1 else [3]


def _planted(rng, script, T):
  """Frame t boosts label t of the script by 12 (the cursor climbs two states per frame), the frames behind the script its blank."""
  x = rng.standard_normal((T, C)).astype(np.float32)
  for t in range(T):
    x[t, script[t] if t < len(script) else C - 1] += np.float32(12.0)
  return x


def _both(scripts, K, dev, max_events=256, max_rows=400, max_labels=1000):
  starts = [FO.word_starts(s, SPACE) for s in scripts]
  return (Driver(scripts, starts, C, max_labels, K, max_events=max_events, max_rows=max_rows),
          Driver(scripts, starts, C, max_labels, K, max_events=max_events, max_rows=max_rows, device=dev))


def _same_step(host, device, feeds, **kw):
  h, d = host.step(feeds, **kw), device.step(feeds, **kw)
  for s in h:
    assert np.array_equal(h[s]['record'], d[s]['record']), (s, h[s]['record'], d[s]['record'])
    assert h[s]['events'] == d[s]['events'] and np.array_equal(h[s]['trace'], d[s]['trace']), s
    assert host.state_bytes(s).tobytes() == device.state_bytes(s).tobytes(), 'state of slot {}'.format(s)
  return h


def _feed_same(host, device, streams, cuts):
  at = {s: 0 for s in streams}
  k, events, trace = 0, {s: [] for s in streams}, {s: [] for s in streams}
  while any(at[s] < len(streams[s]) for s in streams):
    feeds = {}
    for s, x in streams.items():
      if at[s] < len(x):
        n = cuts[s][k % len(cuts[s])]
        feeds[s] = x[at[s]:at[s] + n]
        at[s] += n
    out = _same_step(host, device, feeds)
    for s in feeds:
      events[s] += out[s]['events']
      trace[s] += out[s]['trace'].tolist()
    k += 1
  return events, trace


@pytest.mark.parametrize('L', [1, 447, 448, 895, 896, 1000])
def test_kernel_equals_host_form_at_the_block_edges(dev, L):
  """1, 1, 2, 2, 3 and 3 state blocks: the edges at U = 895 / 897 and 1 791 / 1 793."""
  rng = np.random.default_rng(L)
  script = _script(rng, L)
  assert (2 * L + 1 + 895) // 896 == {1: 1, 447: 1, 448: 2, 895: 2, 896: 3, 1000: 3}[L]
  planted, noise = _planted(rng, script, 950), AO.random_logits(rng, 1000, C)
  host, device = _both([script], 3, dev)
  events, trace = (v[0] for v in _feed_same(host, device, {0: planted}, {0: [64]}))            # runs of exactly 64 rows
  assert trace[:min(L, 950)] == [2 * t + 1 for t in range(min(L, 950))] and events
  if L == 1000:
    assert max(trace) == 1899                                                   # block 2
  for s in (host, device):
    s.reopen(0)
  events, trace = (v[0] for v in _feed_same(host, device, {0: noise}, {0: [130, 1, 65, 7, 64, 63]}))   # 130 rows: three runs in a step
  r = FO.follow64(noise, script, FO.word_starts(script, SPACE), 3)
  if r.margin.min() > 1e-9:
    assert trace == r.c.tolist() and events == r.events


def test_three_streams_with_different_scripts_in_one_launch(dev):
  rng = np.random.default_rng(42)
  scripts = [_script(rng, 1000), [], _script(rng, 447), _script(rng, 1)]       # slot 1 is not followed
  streams = {0: _planted(rng, scripts[0], 700), 1: AO.random_logits(rng, 90, C), 2: AO.random_logits(rng, 520, C),
             3: _planted(rng, scripts[3], 333)}
  host, device = _both(scripts, 16, dev, max_rows=520)
  events, trace = _feed_same(host, device, streams, {0: [130, 64], 1: [30], 2: [64, 1, 128], 3: [100, 0, 11]})
  for s in (0, 2, 3):
    r = FO.follow64(streams[s], scripts[s], FO.word_starts(scripts[s], SPACE), 16)
    assert r.margin.min() > 1e-9
    assert trace[s] == r.c.tolist() and events[s] == r.events
  assert events[0] and trace[1] == [-77] * 90
  # alone, stream 2 leaves the same state and says the same
  alone_h, alone_d = _both([[], [], scripts[2], []], 16, dev, max_rows=520)
  ev2, tr2 = _feed_same(alone_h, alone_d, {2: streams[2]}, {2: [64]})
  assert (ev2[2], tr2[2]) == (events[2], trace[2]) and alone_d.state_bytes(2).tobytes() == device.state_bytes(2).tobytes()


def test_limit_reset_and_sitting_out_on_the_device(dev):
  rng = np.random.default_rng(8)
  script = _script(rng, 500)
  x = _planted(rng, script, 300)
  host, device = _both([script, script[:40]], 2, dev)
  _same_step(host, device, {0: x[:100], 1: x[:10]})
  _same_step(host, device, {1: x[10:20]})                                      # slot 0 sits out
  _same_step(host, device, {0: x[100:250]}, limits={0: 180}, guard=8)          # rows at or past the limit are not consumed
  for s in (host, device):
    s.reopen(0)
  out = _same_step(host, device, {0: x[:0]})                                   # a reset without rows
  assert out[0]['frames'] == 0 and out[0]['c'] == -1
  out = _same_step(host, device, {0: x[:64]})
  assert out[0]['trace'].tolist() == [2 * t + 1 for t in range(64)]


def test_event_overflow_reports_the_true_count(dev):
  rng = np.random.default_rng(2)
  script = FO.script_without_repeats(rng, 120, C, SPACE, word_len=1)
  x = _planted(rng, script, 120)
  host, device = _both([script], 1, dev, max_events=1, max_labels=120)
  out = _same_step(host, device, {0: x}, guard=64)[0]                          # (guard words behind the events and the trace stay)
  assert len(out['events']) == 1 and out['lost'] == 59 and out['words'] == 60
  # a stream with more rows than the caller announced loses them with a status, on both forms
  host, device = _both([script], 1, dev, max_labels=120)
  out = _same_step(host, device, {0: np.concatenate([x, x])}, max_stream_rows=128)[0]
  assert out['frames'] == 128 and out['status'] == 4


def test_bad_arguments_launch_nothing(dev):
  from speecht_amd._lib import launch_trace
  rng = np.random.default_rng(1)
  script = _script(rng, 10)
  _, device = _both([script], 2, dev, max_labels=10)
  device.K = 17
  with launch_trace() as tr:
    with pytest.raises(Exception, match='confirm'):
      device.step({0: AO.random_logits(rng, 5, C)})
  assert tr.lines == []
  assert (device.state_bytes(0) == 0xA5).all()


# ---- the recogniser -------------------------------------------------------------------------------------------------------------------

SMALL = WL.w2l_layers(16, width=24, fc=40)
TEXT = 'the cat sat on a mat and then the cat ran'


@pytest.fixture(scope='module')
def small(dev):
  from speecht_amd.engine import Wav2LetterEngine
  params = WL.xavier_params(SMALL, seed=7)
  params[-1] = (params[-1][0] * 12.0, params[-1][1] * 4.0)        # (peakier posteriors, as the other stream tests use)
  eng = Wav2LetterEngine(SMALL, device=dev)
  eng.set_weights(params)
  return eng


def _follower(**kw):
  from speecht_amd.streaming import ScriptFollower
  return ScriptFollower(max_labels=64, confirm=0.04, trace=True, **kw)


def _solo(eng, x, chunk, follow=None, script=None, **options):
  """One stream alone -> (per step the follower's state without its trace, the trace, the reached words, everything else the steps
  reported, the logits, the recogniser)."""
  from speecht_amd.streaming import StreamingRecognizer
  rec = StreamingRecognizer(eng, 2, max_chunk_frames=64, follow=follow, **options)
  rec.open()
  slot = rec.open(script=script) if follow is not None else rec.open()      # (slot 1: slot 0 stays idle beside it)
  states, trace, reached, rest, rows = [], [], [], [], []
  for at in list(range(0, len(x), chunk)) + ['end']:
    r = rec.finish(slot, return_logits=True) if at == 'end' else rec.step({slot: x[at:at + chunk]}, return_logits=True)
    rows.append(r.logits[slot])
    rest.append((at, r.ids[slot], r.score[slot], r.hyp.get(slot), r.stable.get(slot), r.logp.get(slot), repr(r.finals.get(slot)),
                 r.open_ids.get(slot), repr(r.hits.get(slot))))
    if follow is not None:
      assert r.reached_lost[slot] == 0
      st = dict(r.follow[slot])
      trace += st.pop('trace')
      states.append(st)
      reached += [(w.index, w.text, w.frame) for w in r.reached[slot]]
    else:
      assert r.follow == {} and r.reached == {} and r.reached_lost == {}
  return states, trace, reached, rest, np.concatenate(rows), rec


def _options(which):
  from speecht_amd.streaming import Endpointing, StreamBeam, StreamSpotter
  out = {}
  if 'beam' in which:
    out['beam'] = StreamBeam(beam_width=16, max_seconds=4.0)
  if 'endpoint' in which:
    out['endpoint'] = Endpointing(silence=0.06, lead=0.2, max_utterance=0.6)
  if 'spot' in which:
    out['spot'] = StreamSpotter(['a', 'th'], threshold=-np.inf, hold=0.1, max_events=512)
  return out


@pytest.mark.parametrize('which', ['alone', 'beam', 'endpoint+spot', 'beam+endpoint+spot'])
def test_recogniser_however_the_audio_is_cut_and_beside_the_other_options(dev, small, which):
  x = WL.synthetic_features(151, 151, 16).astype(np.float32)
  st_a, tr_a, re_a, rest_a, logits, rec_a = _solo(small, x, 50, _follower(), TEXT, **_options(which))
  st_b, tr_b, re_b, rest_b, logits_b, _ = _solo(small, x, 25, _follower(), TEXT, **_options(which))
  _, _, _, rest_plain, logits_plain, rec_plain = _solo(small, x, 50, None, None, **_options(which))
  assert np.array_equal(logits, logits_b) and np.array_equal(logits, logits_plain)
  assert tr_a == tr_b and re_a == re_b and st_a[-1] == st_b[-1]
  # what it says is the host form's on the stream's own rows (those past the decode limit are not consumed)
  fw = _follower()
  ids, starts, words = fw.script(TEXT, C)
  K = fw.frames(2)
  assert K == 2 and starts == FO.word_starts(ids, SPACE)
  host = Driver([ids], [starts], C, 64, K, max_rows=len(logits))
  want = host.step({0: logits}, limits={0: 151 // 2})[0]
  assert tr_a == want['trace'][:151 // 2].tolist() and len(tr_a) == 151 // 2
  assert [(j, t) for j, _, t in re_a] == want['events'] and all(text == words[j] for j, text, _ in re_a)
  last = st_a[-1]
  assert (last['frames'], last['state'], last['status']) == (want['frames'], want['c'], 0)
  assert np.float64(last['fit']).view(np.int64) == np.float64(want['fit']).view(np.int64)
  assert np.float64(last['end_score']).view(np.int64) == np.float64(want['end_score']).view(np.int64)
  c = last['state']
  assert last['label'] == ((c - 1) >> 1 if c >= 1 else -1) and last['in_blank'] == (c >= 0 and c % 2 == 0)
  assert last['complete'] == (c >= 2 * len(ids) - 1) and last['fit'] <= 0
  # the decoders, the endpointer and the spotter report what they report without a follower; its launches come on top: the
  # softmax, the tiles and the read-out (the last pass of these cuts has rows)
  assert rest_a == rest_plain and rec_a.launches - rec_plain.launches in (2, 3)
  assert not hasattr(rec_plain, 'follow_state') and rec_plain._follow is None


def _all_options_passes(eng):
  """One stream with every option on, two steps of 64 frames and `finish` -> per pass (the kernels launched, ``launches``)."""
  from speecht_amd._lib import launch_trace
  from speecht_amd.streaming import Endpointing, FinalWords, StreamBeam, StreamingRecognizer, StreamSpotter
  x = WL.synthetic_features(151, 151, 16).astype(np.float32)
  rec = StreamingRecognizer(eng, 1, max_chunk_frames=64, beam=StreamBeam(beam_width=16, nbest=2),
                            endpoint=Endpointing(silence=0.06, lead=0.2, max_utterance=0.6), words=FinalWords(),
                            spot=StreamSpotter(['a', 'th'], threshold=-np.inf, hold=0.1, max_events=512), follow=_follower())
  slot = rec.open(script=TEXT)
  passes = []
  for run in (lambda: rec.step({slot: x[:64]}), lambda: rec.step({slot: x[64:128]}), lambda: rec.finish(slot)):
    with launch_trace() as tr:
      run()
    passes.append(([l.split(' ')[0] for l in tr.lines], rec.launches))
  return passes


# (22 pieces per pass; the first pass has rows in seven layers and none for the decoders; `finish` closes an utterance with words)
_DECODERS = (['ctc_greedy_endpoint_stream'] + ['ctc_beam_stream<wave>', 'ctc_beam_stream_read_nbest<wave>'] * 22
             + ['ctc_spot_stream<1>', 'ctc_follow_stream'])
_PRODUCTS = ['stream_conv<32>'] * 8 + ['stream_conv<64>'] * 2 + ['stream_conv<32>', 'stream_keep']
ALL_OPTIONS_PASSES = [(['stream_conv<32>'] * 7 + _DECODERS, 66), (_PRODUCTS + _DECODERS, 77),
                      (_PRODUCTS + _DECODERS + ['ctc_align_ring<1>'], 79)]


def test_all_options_launch_what_they_launched(dev, small):
  """The kernels of each pass, in order, and ``launches``: recorded by running `_all_options_passes` on the commit before the options
  owned their parts of a pass, on this file's tiny engine.  (The trace does not name the feed and the advance: of those only
  ``launches`` tells.)"""
  assert _all_options_passes(small) == ALL_OPTIONS_PASSES


def test_follow_none_takes_the_old_path(dev, small):
  from speecht_amd._lib import launch_trace
  from speecht_amd.streaming import StreamError, StreamingRecognizer
  x = WL.synthetic_features(77, 151, 16).astype(np.float32)       # three passes of up to 64 frames

  def traced(follow, script):
    rec = StreamingRecognizer(small, 2, max_chunk_frames=64, follow=follow)
    slot = rec.open(script=script) if script else rec.open()
    with launch_trace() as tr:
      r = rec.step({slot: x})
    return tr.lines, rec, r.ids[slot]

  plain, rec_plain, ids_plain = traced(None, None)
  with_f, rec_f, ids_f = traced(_follower(), TEXT)
  assert ids_plain == ids_f
  assert not any('follow' in l for l in plain) and sum('ctc_follow_stream' in l for l in with_f) == 3
  assert [l for l in with_f if 'ctc_follow_stream' not in l] == plain
  S = 2
  assert rec_plain.dec_out.numel() == S * rec_plain.max_new + 2 * S          # the buffers of a recogniser without options
  assert rec_f.dec_out.numel() == rec_plain.dec_out.numel() + S * (16 + 2 * 64) + rec_f.max_rows[-1]
  with pytest.raises(StreamError, match='ScriptFollower'):
    rec_plain.open(script=TEXT)
  with pytest.raises(StreamError, match='follower'):
    rec_f.step({}, fetch=False)
  # a stream opened without a script beside a followed one is not followed; a reused slot starts its script over
  rec = StreamingRecognizer(small, 2, max_chunk_frames=64, follow=_follower())
  a, b = rec.open(script=TEXT), rec.open()
  r = rec.step({a: x, b: x})
  assert b not in r.follow and r.follow[a]['frames'] == len(r.follow[a]['trace']) > 0
  first = r.follow[a]
  rec.close(a)
  a2 = rec.open(script=TEXT)
  r2 = rec.step({a2: x})
  assert a2 == a and r2.follow[a2] == first
