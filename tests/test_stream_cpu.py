"""Streaming recognition without a GPU: the float64 statement of the feature (tests/stream_oracle.py) against the oracle's
whole-utterance forward pass and greedy decoder, and the index arithmetic of speecht_amd/streaming.py against a brute-force
enumeration of receptive fields; the layout of a step's result buffer for every set of options, and the beam search's read-out."""
import numpy as np
import pytest

from oracle import w2l_oracle as O
from tests import stream_oracle as SO
from tests.workloads import synthetic_features, w2l_layers, xavier_params

LENGTHS = (1, 2, 3, 47, 48, 97, 98, 99, 150, 151)
LAYERS = w2l_layers(16, width=24, fc=40)
GEO = [(l[0], l[1]) for l in LAYERS]


@pytest.fixture(scope='module')
def params():
  return xavier_params(LAYERS, seed=7)


@pytest.mark.parametrize('T', LENGTHS)
def test_state_machine_reproduces_the_whole_utterance(params, T):
  x = synthetic_features(T, T, 16)
  ref = O.wav2letter_forward(x[None], params, LAYERS)[:, 0]
  ref_ids, ref_score = O.ctc_greedy_decode(ref[:, None], [T // 2])
  for name, chunks in SO.chunkings(T).items():
    logits, ids, first_at, model = SO.run_stream(params, LAYERS, x, chunks)
    assert logits.shape == ref.shape, name
    assert np.max(np.abs(logits - ref)) < 1e-12, name
    assert ids == ref_ids[0], name
    assert abs(model.greedy.score - ref_score[0, 0]) < 1e-9, name
    assert model.greedy.frames == T // 2
    # no row before 99 input frames, the first at 99 (or at finish when the utterance is shorter)
    if name == 'ones':
      assert first_at == (99 if T >= 99 else T), (T, first_at)
    else:
      assert first_at >= min(99, T), (name, first_at)
    for l in model.layers:
      assert l.e == -(-l.n // l.stride)
      if name == 'ones':                                         # fed frame by frame a layer never keeps more than its width
        assert l.max_kept <= l.width + l.stride


def test_first_row_and_lag_from_the_plan():
  from speecht_amd import streaming
  assert streaming.first_row_after(GEO) == (99, 49)
  assert streaming.first_row_after([(l[0], l[1]) for l in w2l_layers(80)]) == (99, 49)


def test_greedy_across_steps_constructed():
  x, expect = SO.greedy_case()
  T = len(x)
  ref_ids, ref_score = O.ctc_greedy_decode(x[:, None], [T])
  assert ref_ids[0] == expect
  for step in (1, 2, 3, T):
    g = SO.GreedyStream(5)
    ids = []
    for at in range(0, T, step):
      ids += g.push(x[at:at + step])
    assert ids == expect and g.score == ref_score[0, 0] and g.frames == T
  # a decode limit known only at the end: the rows from it on are not taken
  g = SO.GreedyStream(5)
  ids = g.push(x[:10]) + g.push(x[10:], limit=12)
  assert ids == O.ctc_greedy_decode(x[:, None], [12])[0][0] and g.frames == 12


def test_left_padding_does_not_depend_on_the_length():
  from speecht_amd import streaming
  for width, stride in sorted(set(GEO)):
    assert streaming.pad_left_fixed(width, stride)
    for T in range(1, 261):
      t_out, pl, pr = O.same_padding(T, width, stride)
      assert pl == streaming.pad_left(width, stride) == SO.pad_left(width, stride), (width, stride, T)
  assert not streaming.pad_left_fixed(5, 3) and not streaming.pad_left_fixed(3, 2) and not streaming.pad_left_fixed(1, 2)


def _brute(width, stride, n, finished):
  """Ready outputs and the first input frame still needed, by enumerating every output's receptive field."""
  pl = SO.pad_left(width, stride)
  ready = []
  for j in range(0, n + 2):
    field = [j * stride - pl + w for w in range(width)]
    if finished:
      ok = j < -(-n // stride)
    else:
      ok = max(field) <= n - 1
    if ok:
      ready.append(j)
  assert ready == list(range(len(ready)))
  nxt = len(ready)
  need = min(t for t in [nxt * stride - pl + w for w in range(width)])
  return len(ready), max(need, 0)


def test_plan_against_receptive_fields():
  from speecht_amd import streaming
  for width, stride in sorted(set(GEO)) + [(6, 2), (4, 2), (2, 1)]:
    for n in range(0, 261):
      for fin in (False, True):
        count, need = _brute(width, stride, n, fin)
        assert streaming.ready_count(n, width, stride, fin) == count, (width, stride, n, fin)
        assert streaming.retain_from(count, width, stride) == need
        assert streaming.emit_count(n, max(count - 2, 0), width, stride, fin) == min(count, 2)
  for T in range(0, 261):
    assert streaming.decode_limit(T) == T // 2


@pytest.mark.parametrize('chunk', (1, 7, 20, 64))
def test_plan_chains_the_layers_for_every_length(chunk):
  from speecht_amd import streaming
  bound = streaming.max_new_frames(GEO, chunk)
  for T in list(range(1, 261, 1 if chunk > 1 else 13)):
    n, e = [0] * len(GEO), [0] * len(GEO)
    seen = [[] for _ in GEO]
    fed = 0
    while True:
      new = min(chunk, T - fed)
      fin = new == 0
      steps, n, e = streaming.plan(GEO, n, e, new, fin)
      fed += new
      for l, (first, count, base, n_l, new_base) in enumerate(steps):
        width, stride = GEO[l]
        assert count <= bound[l + 1], (T, l, count)
        assert n_l - base <= width + bound[l]                    # the window the session allocates
        for j in range(first, first + count):                    # every tap of an emitted row is stored, padding or beyond the end
          for t in (j * stride - streaming.pad_left(width, stride), j * stride - streaming.pad_left(width, stride) + width - 1):
            assert t < 0 or t >= n_l or t >= base
          if not fin:
            assert j * stride - streaming.pad_left(width, stride) + width - 1 <= n_l - 1
        seen[l] += range(first, first + count)
        assert new_base == streaming.retain_from(first + count, width, stride) and new_base <= max(n_l, 0)
      if fin:
        break
    t = T
    for l, (width, stride) in enumerate(GEO):
      t = -(-t // stride)
      assert seen[l] == list(range(t)), (T, l)


def test_library_exports_the_streaming_entry_points():
  from speecht_amd import _lib
  lib = _lib.load()
  for name in ('st_stream_conv_slices', 'st_stream_conv_ws', 'st_stream_conv_f32', 'st_stream_feed_f32', 'st_stream_advance',
               'st_ctc_greedy_stream'):
    assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS, name
  # the slices of the reduction are a function of the layer's shape alone; the workspace grows with the rows only
  import ctypes
  kt, sl = ctypes.c_int(), ctypes.c_int()
  for width, cp, cout in ((48, 80, 250), (7, 256, 250), (32, 256, 2000), (1, 2016, 2000), (1, 2016, 29)):
    assert lib.st_stream_conv_slices(width, cp, cout, ctypes.byref(kt), ctypes.byref(sl)) == 0
    k_pad = -(-width * cp // 32) * 32
    assert sl.value >= 1 and kt.value * sl.value >= k_pad // 32 > kt.value * (sl.value - 1)
    n_pad = 32 if cout <= 32 else -(-cout // 128) * 128
    for rows in (1, 33, 640):
      assert lib.st_stream_conv_ws(rows, width, cp, cout) == sl.value * rows * n_pad * 4
  assert lib.st_stream_conv_ws(0, 7, 256, 250) == 0


# ---- the mel front end -------------------------------------------------------------------------------------------------------

def test_features_short_utterance_and_fixed_statistics_equal_offline():
  sr, n_mels = 16000, 40
  short = O.synthetic_audio(31, 160 * 57 + 33).astype(np.float64)          # 58 frames <= warm
  ref = O.calc_power_spectrogram(short, sr, n_mels=n_mels)
  for chunks in ([len(short)], [1600] * 5, [3217, 0, 100]):
    got = SO.stream_features(sr, n_mels, short, chunks)
    assert got.shape == ref.shape and np.max(np.abs(got - ref)) < 1e-9
  exact = O.synthetic_audio(33, 160 * 99 + 5).astype(np.float64)           # exactly warm frames
  assert np.max(np.abs(SO.stream_features(sr, n_mels, exact, [4000]) - O.calc_power_spectrogram(exact, sr, n_mels=n_mels))) < 1e-9
  long = O.synthetic_audio(32, 160 * 130 + 7).astype(np.float64)           # 131 frames > warm
  ref = O.calc_power_spectrogram(long, sr, n_mels=n_mels)
  got = SO.stream_features(sr, n_mels, long, [1600] * 9, stats=SO.file_statistics(sr, n_mels, long))
  assert got.shape == ref.shape and np.max(np.abs(got - ref)) < 1e-9
  # running statistics on the long one: independent of the chunking, the first warm frames as the first warm frames alone
  a = SO.stream_features(sr, n_mels, long, [1600] * 9)
  b = SO.stream_features(sr, n_mels, long, [len(long)])
  assert a.shape == ref.shape and np.max(np.abs(a - b)) < 1e-12
  assert np.max(np.abs(a - ref)) > 1e-3                                    # causal statistics are not the file's
  S = O.mel_filterbank(sr, 512, n_mels) @ O.stft_power(long, 512, 160)
  head = O.normalize(O.power_to_db(S[:, :100])).T
  assert np.max(np.abs(a[:100] - head)) < 1e-9


def test_feature_plan_twin():
  from speecht_amd import streaming
  for n in range(0, 2000, 7):
    ready = sum(1 for t in range(0, 40) if t * 160 + 255 <= n - 1 and 256 - t * 160 <= n - 1)
    assert streaming.frames_ready(n, 160, False) == ready - ready % 2, n
    if n > 256:
      assert streaming.frames_ready(n, 160, True) == 1 + n // 160
  assert streaming.sample_base(0, 160) == 0 and streaming.sample_base(2, 160) == 64 and streaming.sample_base(10, 160) == 1344


# ---- the command line ----------------------------------------------------------------------------------------------------------

def _cli():
  import importlib.machinery
  import importlib.util
  import os
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  loader = importlib.machinery.SourceFileLoader('speecht_cli_stream', os.path.join(root, 'speecht-cli'))
  spec = importlib.util.spec_from_loader('speecht_cli_stream', loader)
  cli = importlib.util.module_from_spec(spec)
  loader.exec_module(cli)
  return cli


def test_cli_stream_parses_and_record_still_exits_2(capsys):
  cli = _cli()
  _, flags = cli.parse(['stream', 'a.flac'])
  assert (flags.command, flags.path, flags.chunk_ms, flags.normalize, flags.sample_rate) == ('stream', 'a.flac', 200.0, 'running', 16000)
  assert flags.feature_type == 'power' and flags.run_type == 'other'
  _, flags = cli.parse(['stream', '-', '--sample-rate', '8000', '--chunk-ms', '50', '--normalize', 'file', '--run-name', 'r'])
  assert (flags.path, flags.sample_rate, flags.chunk_ms, flags.normalize, flags.run_train_dir) == ('-', 8000, 50.0, 'file', 'train/r')
  for bad in (['stream'], ['stream', 'a.flac', '--normalize', 'offline'], ['stream', 'a.flac', '--chunk-ms', '0']):
    with pytest.raises(SystemExit) as e:
      cli.main(bad)
    assert e.value.code == 2
  capsys.readouterr()
  assert cli.main(['record']) == 2
  assert 'not part of the MI355X hot path' in capsys.readouterr().out


def test_pcm_chunks_from_a_byte_stream():
  import io
  from speecht_amd import streaming
  pcm = (np.arange(-5, 6) * 1000).astype('<i2')
  got = list(streaming._pcm_chunks(io.BytesIO(pcm.tobytes() + b'\x01'), 4))       # a trailing odd byte is dropped
  assert [len(g) for g in got] == [4, 4, 3]
  assert np.array_equal(np.concatenate(got), pcm.astype(np.float32) / 32768.0)


def test_plan_many_equals_plan():
  from speecht_amd import streaming
  rng = np.random.default_rng(5)
  k = 7
  n, e = np.zeros((k, len(GEO)), np.int64), np.zeros((k, len(GEO)), np.int64)
  done = np.zeros(k, bool)
  for step in range(40):
    new = rng.integers(0, 30, k) * ~done
    fin = (rng.random(k) < 0.05) & ~done & (n[:, 0] + new > 0)
    new[fin] = 0
    first, count, base, n_after, new_base = streaming.plan_many(GEO, n, e, new, fin)
    for i in range(k):
      steps, n_i, e_i = streaming.plan(GEO, n[i].tolist(), e[i].tolist(), int(new[i]), bool(fin[i]))
      assert steps == [tuple(int(v[i, l]) for v in (first, count, base, n_after, new_base)) for l in range(len(GEO))]
      assert n_i == n_after[i].tolist() and e_i == (first[i] + count[i]).tolist()
    n, e = n_after, first + count
    done |= fin


def test_step_layout_orders_the_result_buffer_for_every_set_of_options():
  """All 32 sets of {endpoint, beam, spot, follow with trace, lists}; lists need a beam, one piece without endpointing."""
  import itertools
  from speecht_amd.streaming import StepLayout
  S, NEW, TAIL, SPOT, FOLLOW, ROWS = 3, 5, 7, 3, 2, 15
  order = ['ids', 'counts', 'scores', 'events', 'pieces', 'result', 'tail', 'spot_counts', 'spot_events', 'follow_records',
           'follow_events', 'follow_trace', 'used']
  assert StepLayout(S, NEW).size == 21
  parities, seen = set(), 0
  for ep, beam, spot, follow, lists in itertools.product([False, True], repeat=5):
    if lists and not beam:
      continue
    seen += 1
    P = 2 if ep else 1
    lay = StepLayout(S, NEW, n_pieces=P if ep else None, max_tail=TAIL if beam else None, spot_events=SPOT if spot else None,
                     follow_events=FOLLOW if follow else None, trace_rows=ROWS if follow else None, lists=lists)
    names = list(lay.segments)
    assert names == [n for n in order if n in names]
    assert set(names) == ({'ids', 'counts', 'scores'} | ({'events', 'pieces'} if ep else set()) | ({'result', 'tail'} if beam else set())
                          | ({'spot_counts', 'spot_events'} if spot else set()) | ({'used'} if lists else set())
                          | ({'follow_records', 'follow_events', 'follow_trace'} if follow else set()))
    end = 0
    for name in names:                                            # contiguous and disjoint, but for the follower's even start
      first, length, shape = lay.segments[name]
      assert length == int(np.prod(shape)) > 0
      if name == 'follow_records':
        parities.add(end & 1)
        assert first == end + (end & 1) and first % 2 == 0
      else:
        assert first == end, name
      end = first + length
    assert end == lay.size
    if lists:
      assert lay.segments['used'] == (lay.size - 1, 1, (1,))
    total = S * NEW + S + S                                        # the sizes, written out again
    total += S * P * 8 + P * S * 4 if ep else 0
    total += P * S * 4 + P * S * TAIL if beam else 0
    total += S + S * SPOT * 8 if spot else 0
    total += total % 2 + S * 16 + S * FOLLOW * 2 + ROWS if follow else 0
    total += 1 if lists else 0
    assert lay.size == total, (ep, beam, spot, follow, lists)
    words = np.arange(lay.size, dtype=np.int32)                    # a view is its segment of the words, in its shape
    for name in names:
      first, length, shape = lay.segments[name]
      view, = lay.views(name)(words)
      assert view.shape == shape and view.reshape(-1).tolist() == list(range(first, first + length))
  assert seen == 24 and parities == {0, 1}
  assert not StepLayout(S, NEW, follow_events=FOLLOW).segments.keys() & {'follow_trace'}
  max_new = 11
  assert StepLayout(1, max_new, max_tail=256).size == max_new + 2 + 4 + 256


def test_read_beam_on_hand_written_rows():
  from speecht_amd.streaming import read_beam
  logp = np.float32(-3.25)
  row = lambda length, stable, status=0: np.asarray([length, stable, int(logp.view(np.int32)), status], dtype=np.int32)
  tail = np.asarray([7, 8, 9, 0, 0], dtype=np.int32)
  hyp = [1, 2, 3, 4]
  # two ids are final; the device reports five in all, three of them final now: the tail goes above the two
  got = read_beam(hyp, 2, row(5, 3), tail, 5, False)
  assert got[0] == [1, 2, 7, 8, 9] and got[1] == 3 and got[3] == [1, 2] and hyp == [1, 2, 3, 4]
  assert isinstance(got[2], np.float32) and got[2].tobytes() == logp.tobytes()
  assert read_beam(hyp, 2, row(5, 3), tail, 5, True)[:2] == ([1, 2, 7, 8, 9], 5)       # a final is final as a whole
  assert read_beam(hyp, 2, row(2, 2), tail, 5, False)[:2] == ([1, 2], 2)               # nothing above the stable ids
  assert read_beam([], 0, row(0, 0), tail, 5, True)[:2] == ([], 0)
  assert read_beam(hyp, 2, row(5, 3, status=6), tail, 5, False) == 'status 6'
  assert read_beam(hyp, 2, row(8, 3), tail, 5, False) == '6 labels are not final yet, max_tail = 5'
  assert isinstance(read_beam(hyp, 2, row(7, 3), np.arange(5, dtype=np.int32), 5, False), tuple)    # exactly max_tail labels fit
  assert isinstance(read_beam(hyp, 3, row(2, 2), tail, 5, False), str)                 # shorter than what is final already
