#!/usr/bin/env python3
"""N-best lists and second-pass rescoring for the finals of live streams (StreamBeam(nbest=, rescore=),
st_ctc_beam_stream_read_nbest / _step_pieces_nbest): what they cost.  By the protocol of scripts/bench_stream_beam.py part (c) and
scripts/bench_endpoint.py: the full-size 80-mel model, 200 ms of audio per stream and step, 1 / 16 / 64 streams, the synthetic
200 k / 1 M / 1 M trigram of scripts/bench_lm_decode.py, the forms alternating inside every round.  No threshold is fixed in advance:
every ratio comes with the spread of its baseline's own repeats (max / min of the baseline), and `inside` says whether the ratio's
median lies within it.

  read_out   the finishing read-out alone, 64 streams: st_ctc_beam_stream_read_nbest with n_best 1 / 10 / beam against
             st_ctc_beam_stream_read on the same records (beam 100 with the model, beam 16 without), microseconds per call;
  quiet      a step in which nothing finishes, lists on against off: with and without endpointing;
  events     an endpoint every 3 s of every stream (every row is speech, max_utterance = 3 s): lists off / lists / lists and
             rescoring, and the cost per final;
  two_pass   beam 16 LM-free with nbest = 16 rescored under the trigram against beam 100 with the trigram in the first pass, both
             with an endpoint every 3 s: step time and streams in real time.  The COST side only: the model is random and there is no
             data, so nothing here says what either does for accuracy.

  existing   with --parent DIR (a built tree of the commit before): the plain beam-16 step, the endpointed beam-100 step,
             st_ctc_beam_stream_read and st_ctc_beam_search_decode_lm_nbest (16 streams, a 20 k / 100 k / 100 k trigram) and bench.py,
             --repeats processes per tree, alternating; every ratio beside the parent's own max / min over its repeats.

read_out also runs the N-best read-out with an arena of 0 words (no record fits: only `tail` is stored, as in the plain read-out) and
reports how many labels of every stream are not stable yet: the launch is bound by the stream with the most.

Writes profiles/stream_nbest.json (--output)."""
import argparse, ctypes, json, os, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'stream_nbest.json'))
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--streams', type=int, nargs='+', default=[1, 16, 64])
ap.add_argument('--unigrams', type=int, default=200000)
ap.add_argument('--bigrams', type=int, default=1000000)
ap.add_argument('--trigrams', type=int, default=1000000)
ap.add_argument('--parent', default=None, help='a built tree of the parent commit: also measure `existing`')
ap.add_argument('--repeats', type=int, default=3, help='existing: processes per tree')
ap.add_argument('--bench-steps', type=int, default=20)
ap.add_argument('--existing-child', default=None, metavar='TREE', help='(internal) measure the existing paths of TREE, print one JSON line')
a = ap.parse_args()
TREE = os.path.abspath(a.existing_child) if a.existing_child else ROOT
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(TREE, 'scripts'))
import torch  # noqa: E402
import bench_lm_decode as BL  # noqa: E402
from speecht_amd import _lib  # noqa: E402
from speecht_amd._lib import call  # noqa: E402
from speecht_amd.engine import Wav2LetterEngine  # noqa: E402
from speecht_amd.language_model import LanguageModel  # noqa: E402
from speecht_amd.streaming import Endpointing, StreamBeam, StreamingRecognizer  # noqa: E402
from tests.workloads import synthetic_features, w2l_layers  # noqa: E402
if not torch.cuda.is_available():
  sys.exit('bench_stream_nbest.py needs a GPU')
dev = torch.device('cuda:0')
NEW = 20                       # input frames per step: 200 ms


def clock(fn, calls):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(calls):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / calls * 1e3


def spread(v):
  return dict(median=round(sorted(v)[len(v) // 2], 5), min=round(min(v), 5), max=round(max(v), 5))


def against(new, base):
  """The ratio new / base round by round, beside the spread of the baseline's own repeats."""
  ratio = spread([p / q for p, q in zip(new, base)])
  own = max(base) / min(base)
  return dict(ratio=ratio, baseline_max_over_min=round(own, 5), inside=bool(1.0 / own <= ratio['median'] <= own))


def synthetic_model(unigrams, bigrams, trigrams):
  text, _ = BL.synthetic_arpa(1234, unigrams, bigrams, trigrams)
  with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, 'synthetic.arpa')
    with open(path, 'w') as f:
      f.write(text)
    return LanguageModel(path)


def speech_engine():
  eng = Wav2LetterEngine(w2l_layers(80), device='cuda:0')
  eng.init_xavier(42)
  weights = [(np.asarray(F), np.array(b)) for F, b in eng.get_weights()]
  weights[-1][1][-1] -= 1000.0                                    # the blank never wins: every row is speech
  eng.set_weights(weights)
  return eng


def read_call(eng, rec, S):
  """-> the arguments of st_ctc_beam_stream_read on ``rec``'s records with every stream finishing and no new rows."""
  bm, part = rec.beam, rec._beam
  table = np.zeros((S, 4), np.int32)
  table[:, 2] = part.frames
  d_table = torch.from_numpy(table).to(dev)
  return (eng._ptr(d_table), S, bm.beam_width, part.lm_handle, bm.lm_weight, bm.word_count_weight, bm.valid_word_count_weight, bm.oov_score,
          eng._ptr(part.state), eng._ptr(part.pool), rec.max_frames, eng._ptr(part.tail), bm.max_tail, eng._ptr(part.result),
          eng.stream_ptr), d_table


def existing_child():
  """existing, one process: paths that were there before, in the tree this process imports (only what the parent has is used)."""
  assert os.path.realpath(_lib.__file__).startswith(os.path.realpath(TREE)), _lib.__file__
  S = 16
  small = synthetic_model(20000, 100000, 100000)
  eng = speech_engine()
  x = np.stack([synthetic_features(s, 4000, 80) for s in range(S)]).astype(np.float32)

  def stepper(rec):
    slots, at = [rec.open() for _ in range(S)], [0]

    def step():
      if at[0] + NEW > x.shape[1]:
        at[0] = 0
      rec.step({slots[s]: x[s, at[0]:at[0] + NEW] for s in range(S)})
      at[0] += NEW
    for _ in range(8):
      step()
    return step
  plain = stepper(StreamingRecognizer(eng, S, max_chunk_frames=NEW, beam=StreamBeam(beam_width=16, max_seconds=120.0, max_tail=2048)))
  endpointed = stepper(StreamingRecognizer(eng, S, max_chunk_frames=NEW, beam=StreamBeam(lm=small, max_seconds=120.0, max_tail=2048),
                                           endpoint=Endpointing(silence=0.5, lead=1.0, max_utterance=3.0)))
  rec = StreamingRecognizer(eng, S, max_chunk_frames=NEW, beam=StreamBeam(lm=small, max_seconds=30.0, max_tail=2048))
  fill = stepper(rec)
  for _ in range(40):
    fill()
  args, keep = read_call(eng, rec, S)
  read = lambda: call('st_ctc_beam_stream_read', *args)
  off = Wav2LetterEngine([(1, 1, 16, 29, False)], device='cuda:0')
  logits = (np.random.default_rng(5).standard_normal((16, 300, 29)) * 2).astype(np.float32)
  off.load_batch(np.zeros((16, 300, 16)), [300] * 16)
  off.X[-1].interior().copy_(torch.as_tensor(logits))
  off.ctc_lens = torch.as_tensor(np.full(16, 300, np.int32)).to(dev)
  lists = lambda: off.lm_beam_search_decode_nbest(small, 10, 100)
  torch.cuda.synchronize()
  read()
  lists()
  t = dict(plain_step_ms=[], endpoint_beam100_step_ms=[], stream_read_us=[], lm_nbest_ms=[])
  for _ in range(5):
    t['plain_step_ms'].append(clock(plain, 20))
    t['endpoint_beam100_step_ms'].append(clock(endpointed, 20))
    t['stream_read_us'].append(clock(read, 200) * 1e3)
    t['lm_nbest_ms'].append(clock(lists, 5))
  print('CHILD ' + json.dumps({k: sorted(v)[len(v) // 2] for k, v in t.items()}), flush=True)


if a.existing_child:
  existing_child()
  sys.exit(0)

lm = synthetic_model(a.unigrams, a.bigrams, a.trigrams)
lib = _lib.load()
out = dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, model=dict(lm.info, synthetic_seed=1234),
           timing='host clock around 20 steps (read_out: 200 calls) that end in a device synchronise; the forms alternate inside every '
                  'round; `inside`: the median ratio lies within max / min of the baseline\'s own repeats',
           accuracy='not measured: the acoustic model is random and there is no data; two_pass is the cost side only',
           code_identity_by_hand=('by hand, not by this script (hipcc --cuda-device-only -S on both trees): device assembly of '
                                  "csrc/ctc_beam.hip, this build against the parent, compared per kernel with the block labels' numbers"
                                  ' normalised: all 52 ctc_beam_kernel / log-softmax instantiations and six of the eight '
                                  'ctc_beam_read_kernel instantiations are identical instruction for instruction; the two LM-free '
                                  'biased read-outs (<64, false, true> and <128, false, true>) hold the same instructions with one '
                                  'adjacent independent pair (a v_lshlrev_b32 and a v_lshl_add_u64) in the other order'),
           earlier_forms_by_hand='two figures DESIGN.md quotes come from earlier forms of the read-out, timed once with this script\'s '
                                 'read_out part and not reproducible from this tree: hypothesis 0\'s chain walked twice (once for `tail`, '
                                 'once for the arena) 116.0 us at beam 16, n_best 1; the counter zeroed by hipMemsetAsync instead of a '
                                 'one-word launch 37.2 / 119.9 us at beam 100 / beam 16, n_best 1')

eng = speech_engine()
ptr = eng._ptr

# ---- the finishing read-out alone ------------------------------------------------------------------------------------------------
S = 64
x = np.stack([synthetic_features(s, 4000, 80) for s in range(S)]).astype(np.float32)
res = []
for name, make in (('beam100_lm', lambda: StreamBeam(lm=lm, max_seconds=30.0, max_tail=2048)),
                   ('beam16_free', lambda: StreamBeam(beam_width=16, max_seconds=30.0, max_tail=2048))):
  rec = StreamingRecognizer(eng, S, max_chunk_frames=NEW, beam=make())
  slots = [rec.open() for _ in range(S)]
  for at in range(0, 60 * NEW, NEW):                              # 12 s of every stream
    last = rec.step({slots[s]: x[s, at:at + NEW] for s in range(S)})
  unstable = sorted(len(last.hyp[s]) - last.stable[s] for s in slots)
  bm, W = rec.beam, rec.beam.beam_width
  common, d_table = read_call(eng, rec, S)                        # every stream finishing, no new rows: the tail of the utterance
  arena_words = S * (6 + W * (2 + bm.max_tail))
  arena = torch.zeros(arena_words, dtype=torch.int32, device=dev)
  used = torch.zeros(1, dtype=torch.int32, device=dev)
  forms = {'read': lambda: call('st_ctc_beam_stream_read', *common)}
  for n in sorted({1, 10, W}):
    forms['nbest{}'.format(n)] = lambda n=n: call('st_ctc_beam_stream_read_nbest', *common, None, None, n, ptr(arena), arena_words, ptr(used))
  forms['nbest1_arena_of_0_words'] = lambda: call('st_ctc_beam_stream_read_nbest', *common, None, None, 1, ptr(arena), 0, ptr(used))
  torch.cuda.synchronize()
  with torch.cuda.stream(eng.stream):
    for fn in forms.values():                                    # (the first read-out settles the records' stable lengths)
      fn()
    t = {k: [] for k in forms}
    for _ in range(a.rounds):
      for k, fn in forms.items():
        t[k].append(clock(fn, 200) * 1e3)
    demand = {}
    for k, fn in forms.items():
      if k != 'read':
        fn()
        demand[k] = int(used.item())
  r = dict(decoder=name, streams=S, beam=W, frames=int(rec._beam.frames[0]), read_us=spread(t['read']),
           unstable_labels=dict(largest=unstable[-8:], median=unstable[len(unstable) // 2]))
  for k in forms:                                                 # per label of the longest unstable tail, which bounds the launch
    r.setdefault('us_per_label_of_the_longest_tail', {})[k] = round(sorted(t[k])[a.rounds // 2] / max(unstable[-1], 1), 4)
  for k in forms:
    if k != 'read':
      r[k] = dict(us=spread(t[k]), arena_words_used=demand[k], **against(t[k], t['read']))
  print(json.dumps(r), flush=True)
  res.append(r)
  del rec
  torch.cuda.empty_cache()
out['read_out_64_streams'] = res

# ---- whole steps -------------------------------------------------------------------------------------------------------------------
second = dict(language_model=lm)
DECODERS = {
    'beam16_free': lambda **kw: StreamBeam(beam_width=16, max_seconds=120.0, max_tail=2048, **kw),
    'beam100_lm': lambda **kw: StreamBeam(lm=lm, max_seconds=120.0, max_tail=2048, **kw),
}
FORMS = {'off': dict(), 'lists': dict(nbest='beam'), 'rescored': dict(nbest='beam', rescore=second)}
CASES = {'plain': None, 'quiet': Endpointing(silence=0.5, lead=1.0, max_utterance=120.0),
         'events': Endpointing(silence=0.5, lead=1.0, max_utterance=3.0)}
res = []
for case, endpoint in CASES.items():
  for S in a.streams:
    x = np.stack([synthetic_features(s, 4000, 80) for s in range(S)]).astype(np.float32)
    recs, steps, finals = {}, {}, {}
    for name, make in DECODERS.items():
      for form, kw in FORMS.items():
        if form == 'rescored' and case != 'events':
          continue                                                # (without finals nothing is rescored)
        kw = dict(kw)
        if 'nbest' in kw:
          kw['nbest'] = make().beam_width
        rec = StreamingRecognizer(eng, S, max_chunk_frames=NEW, beam=make(**kw), endpoint=endpoint)
        slots = [rec.open() for _ in range(S)]
        at, seen = [0], [0, 0]

        def step(rec=rec, slots=slots, at=at, seen=seen, ep=endpoint):
          if at[0] + NEW > x.shape[1]:
            at[0] = 0
          r = rec.step({slots[s]: x[s, at[0]:at[0] + NEW] for s in range(S)})
          at[0] += NEW
          if ep is not None:
            seen[0] += sum(len(v) for v in r.finals.values())
            seen[1] += sum(r.nbest_lost.values())

        for _ in range(8):
          step()
        recs[name, form], steps[name, form], finals[name, form] = rec, step, seen
    t = {key: [] for key in steps}
    before = {key: finals[key][0] for key in steps}
    for _ in range(a.rounds):                                     # 8 + 5 x 20 steps = 21.6 s of every stream: inside the plain pool
      for key in steps:
        t[key].append(clock(steps[key], 20))
    r = dict(case=case, streams=S, new_frames_per_step=NEW)
    for name in DECODERS:
      d = dict(off_step_ms=spread(t[name, 'off']), launches_per_step={f: recs[name, f].launches for f in FORMS if (name, f) in recs})
      for form in FORMS:
        if form == 'off' or (name, form) not in t:
          continue
        n_finals = finals[name, form][0] - before[name, form]
        extra = (sum(t[name, form]) - sum(t[name, 'off'])) * 20    # ms over all timed steps
        med = sorted(t[name, form])[a.rounds // 2]
        d[form] = dict(step_ms=spread(t[name, form]), finals_in_timed_steps=n_finals, lists_lost=finals[name, form][1],
                       streams_in_real_time=round(S * 0.2 / (med * 1e-3), 1), **against(t[name, form], t[name, 'off']))
        if n_finals:
          d[form]['extra_us_per_final'] = round(extra * 1e3 / n_finals, 2)
      med = sorted(t[name, 'off'])[a.rounds // 2]
      d['off_streams_in_real_time'] = round(S * 0.2 / (med * 1e-3), 1)
      r[name] = d
    if case == 'events':
      cheap, full = t['beam16_free', 'rescored'], t['beam100_lm', 'off']
      r['two_pass'] = dict(beam16_free_nbest16_rescored_ms=spread(cheap), beam100_lm_first_pass_ms=spread(full),
                           streams_in_real_time=dict(two_pass=round(S * 0.2 / (sorted(cheap)[a.rounds // 2] * 1e-3), 1),
                                                     first_pass=round(S * 0.2 / (sorted(full)[a.rounds // 2] * 1e-3), 1)),
                           **against(cheap, full))
    print(json.dumps(r), flush=True)
    res.append(r)
    del recs, steps
    torch.cuda.empty_cache()
out['whole_step_80mel'] = res

if a.parent:
  trees = {'parent': os.path.abspath(a.parent), 'this': ROOT}
  runs = {k: [] for k in trees}
  for _ in range(a.repeats):                                       # alternating processes
    for k, tree in trees.items():
      p = subprocess.run([sys.executable, os.path.abspath(__file__), '--existing-child', tree], capture_output=True, text=True, timeout=600)
      line = [l for l in p.stdout.splitlines() if l.startswith('CHILD ')]
      if p.returncode != 0 or not line:
        sys.exit('the child on {} failed:\n{}\n{}'.format(tree, p.stdout[-2000:], p.stderr[-2000:]))
      r = json.loads(line[0][6:])
      b = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(a.bench_steps), '--warmup', '5'], cwd=tree,
                         capture_output=True, text=True, timeout=900)
      last = [l for l in b.stdout.splitlines() if l.startswith('{')]
      if b.returncode != 0 or not last:
        sys.exit('bench.py in {} failed:\n{}\n{}'.format(tree, b.stdout[-2000:], b.stderr[-2000:]))
      r['bench_py_utterances_per_s'] = json.loads(last[-1])['value']
      runs[k].append(r)
      print(k, json.dumps(r), flush=True)
  paths = {}
  for k in runs['this'][0]:
    mine, theirs = [r[k] for r in runs['this']], [r[k] for r in runs['parent']]
    med = sorted(mine)[len(mine) // 2]
    paths[k] = dict(this=spread(mine), parent=spread(theirs), ratio_this_over_parent=round(med / sorted(theirs)[len(theirs) // 2], 4),
                    parent_max_over_min=round(max(theirs) / min(theirs), 4), inside=bool(min(theirs) <= med <= max(theirs)))
  out['existing_paths_vs_parent'] = dict(streams=16, repeats=a.repeats, order='the parent first in every pair',
                                         model='synthetic 20 k / 100 k / 100 k trigram', paths=paths)

os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
with open(a.output, 'w') as f:
  json.dump(out, f, indent=1)
  f.write('\n')
