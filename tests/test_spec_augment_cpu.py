"""SpecAugment without a GPU: the host form of the library (st_spec_augment_host / st_spec_augment_plan_host through ctypes: the
arithmetic the kernel shares, csrc/spec_augment_core.h) against the numpy specification tests/spec_augment_oracle.py -- the
generator's known answers, plans integer for integer, the applied values, identity, independence of the batch, the draw ids of
data-parallel ranks, and the surface (exports, argument checks, CLI flags)."""
import ctypes
import importlib.machinery
import importlib.util
import os
import re

import numpy as np
import pytest

from tests import spec_augment_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Random123's known answers for Philox4x32-10, recomputed from the definition: (counter, key) -> output
KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]

LD = (80, 27, 2, 100, 2, 1.0)
LD_SMALL = (4, 5, 2, 6, 2, 1.0)


def A():
  from speecht_amd import augmentation
  return augmentation


def lib_plans(policy, seed, ids, lens, C):
  return A().plan_host(A().SpecAugment(policy, seed, ids), lens, C)


def signed(v):
  """A 64-bit pattern as the int64 the draw-id arrays hold."""
  v &= 2 ** 64 - 1
  return v - 2 ** 64 if v >= 2 ** 63 else v


def test_philox_known_answers():
  for counter, key, want in KNOWN:
    assert tuple(O.philox4x32_10(counter, key)) == want
  # ... and the library's generator: with L - 2W - 2 = 2^16 - 1 and 2W = 2^16 - 2 the plan's c and w are the top 16 bits of words 0
  # and 1 of block 0, whose counter is {draw id, 0, 0} and whose key is the seed -- the first known answer, and the third one's key
  W = 2 ** 15 - 1
  L = 2 * W + 2 + 2 ** 16 - 1
  plan = lib_plans((W, 0, 0, 0, 0, 1.0), 0, [0], [L], 80)
  assert plan.tolist() == [[W + 1 + (0x6627e8d5 >> 16), ((0xe169c58d * (2 * W + 1)) >> 32) - W]]
  for counter, key, _ in KNOWN:
    seed, draw_id = key[0] | key[1] << 32, counter[0] | counter[1] << 32
    r = O.philox4x32_10((counter[0], counter[1], 0, 0), key)
    plan = lib_plans((W, 0, 0, 0, 0, 1.0), seed, [signed(draw_id)], [L], 80)
    assert plan.tolist() == [[W + 1 + (r[0] >> 16), ((r[1] * (2 * W + 1)) >> 32) - W]]
    for policy in (LD, LD_SMALL, (3, 90, 8, 50, 8, 0.3)):
      for length in (1, 9, 500):
        assert lib_plans(policy, seed, [signed(draw_id)], [length], 80).tolist() == [O.plan(policy, seed, draw_id, length, 80)]


def plan_cases():
  """(policy, seed, draw id, L, C): every policy at the lengths around the warp's threshold, masks wider than the channels, time
  masks capped below one frame by p L < 1, eight masks of each kind, seeds and ids with high words."""
  rng = np.random.default_rng(2019)
  policies = [LD, LD_SMALL, (80, 27, 1, 100, 1, 1.0), (0, 5, 8, 6, 8, 1.0), (7, 200, 8, 40, 8, 0.2), (3, 20, 3, 1000, 3, 0.01),
              (1, 1, 1, 1, 1, 0.5), (0, 0, 0, 0, 0, 1.0), (5, 0, 2, 0, 2, 0.0), (12, 13, 4, 30, 5, 0.999)]
  cases = []
  for policy in policies:
    W = policy[0]
    lengths = [1, 2, 2 * W + 1, 2 * W + 2, 2 * W + 3, 37, 1001]
    for L in lengths:
      for C in (13, 80, 128):
        for _ in range(10):
          seed = int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2))
          draw_id = int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2)) if rng.integers(0, 2) else int(rng.integers(0, 10 ** 6))
          cases.append((policy, seed, draw_id, L, C))
  return cases


def test_plans_equal_the_specification_and_stay_inside_the_utterance():
  cases = plan_cases()
  assert len(cases) >= 2000
  seen_warp = seen_no_warp = 0
  for policy, seed, draw_id, L, C in cases:
    W, F, mF, T, mT, p = policy
    got = lib_plans(policy, seed, [signed(draw_id)], [L], C)[0].tolist()
    assert got == O.plan(policy, seed, draw_id, L, C), (policy, seed, draw_id, L, C)
    c, w = got[:2]
    if W > 0 and L >= 2 * W + 2:
      seen_warp += 1
      assert W + 1 <= c <= L - W - 1 and -W <= w <= W and 1 <= c + w <= L - 1
      pos = [O.source_position(got, L, t) for t in range(L)]
      s = [i + r / den for i, r, den in pos]
      assert pos[0][:2] == (0, 0) and pos[L - 1][:2] == (L - 1, 0)
      assert pos[c + w][:2] == (c, 0) or c + w == L - 1                  # (the pinned last row, see the oracle)
      assert all(b >= a for a, b in zip(s, s[1:]))
      assert all(i + 1 <= L - 1 for i, r, den in pos if r)               # no row beyond L - 1 is read
    else:
      seen_no_warp += 1
      assert c == 0 and w == 0
    for k in range(mF):
      f0, f = got[2 + 2 * k:4 + 2 * k]
      assert 0 <= f <= min(F, C) and 0 <= f0 and f0 + f <= C
    for k in range(mT):
      t0, t = got[2 + 2 * mF + 2 * k:4 + 2 * mF + 2 * k]
      assert 0 <= t <= min(T, int(np.floor(p * L))) and 0 <= t0 and t0 + t <= L
  assert seen_warp > 300 and seen_no_warp > 300


def test_a_batch_of_plans_is_the_utterances_plans():
  ids = [3, 2 ** 40 + 1, -9, 0]
  lens = [37, 20, 1, 0]
  plans = lib_plans(LD_SMALL, 99, ids, lens, 80)
  for b in range(4):
    assert plans[b].tolist() == O.plan(LD_SMALL, 99, ids[b], lens[b], 80)
  assert np.array_equal(plans[1], lib_plans(LD_SMALL, 99, [ids[1]], [lens[1]], 80)[0])


@pytest.mark.parametrize('channels', [80, 13])
def test_values_against_the_float64_specification(channels):
  """Masked elements are exactly 0; rows at or past L and every element that is not interpolated equal the source bit for bit; an
  interpolated element lies within 4 * 2^-24 * (|x[i]| + |x[i+1]|) of the float64 value.

  The bound: the library forms fl(fl(r / den) * fl(x1 - x0) + x0) with one rounding each for the quotient, the difference and the
  fused multiply-add (r and den are integers below 2^24, exact as floats), u = 2^-24 each:
    q = (r / den)(1 + e1),  d = (x1 - x0)(1 + e2),  result = (q d + x0)(1 + e3).
  With f = r / den in (0, 1): |q d - f (x1 - x0)| <= f |x1 - x0| (2u + u^2) <= (|x0| + |x1|)(2u + u^2), and the last rounding adds
  at most u |q d + x0| <= u (|x0| + |x1|)(1 + 2u + u^2), because f (x1 - x0) + x0 lies between x0 and x1.  Together
  (3u + O(u^2))(|x0| + |x1|) < 4u (|x0| + |x1|); the float64 evaluation adds ~2^-52 of that and is covered by the slack."""
  aug_mod = A()
  rng = np.random.default_rng(channels)
  B, T = 6, 61
  lens = [61, 40, 23, 10, 1, 0]
  x = (rng.standard_normal((B, T, channels)) * rng.uniform(0.1, 30.0, (B, 1, 1))).astype(np.float32)
  interpolated = masked = 0
  for policy in [LD_SMALL, (4, 0, 0, 0, 0, 1.0), (0, 5, 8, 6, 8, 1.0), (9, 100, 3, 30, 2, 0.5)]:
    ids = rng.integers(-2 ** 62, 2 ** 62, B)
    aug = aug_mod.SpecAugment(policy, seed=int(rng.integers(0, 2 ** 62)), draw_ids=ids)
    y, plans = aug_mod.apply_host(aug, x, lens)
    for b in range(B):
      L = lens[b]
      assert plans[b].tolist() == O.plan(policy, aug.seed, int(ids[b]), L, channels)
      ref, kind, lower = O.apply(policy, plans[b].tolist(), x[b], L)
      got = y[b]
      assert np.all(got[kind == 1].view(np.int32) == 0)                                            # +0.0, not merely == 0
      src = x[b][lower]                                                                            # the source row each row reads
      assert np.array_equal(got[kind == 0].view(np.int32), src[kind == 0].view(np.int32))
      assert np.array_equal(got[L:].view(np.int32), x[b, L:].view(np.int32)) and np.all(kind[L:] == 0)
      if plans[b, 0] == 0:
        assert not np.any(kind == 2)
      sel = kind == 2
      if np.any(sel):
        upper = x[b][np.minimum(lower + 1, T - 1)]
        bound = 4.0 * 2.0 ** -24 * (np.abs(src.astype(np.float64)) + np.abs(upper.astype(np.float64)))
        err = np.abs(got.astype(np.float64) - ref)
        assert np.all(err[sel] <= bound[sel]), float(np.max(err[sel] / np.maximum(bound[sel], 1e-300)))
      interpolated += int(np.sum(sel))
      masked += int(np.sum(kind == 1))
  assert interpolated > 1000 and masked > 1000


def test_identity_policy_is_the_copy_bit_for_bit():
  aug_mod = A()
  rng = np.random.default_rng(4)
  x = rng.standard_normal((3, 37, 80)).astype(np.float32)
  x[0, 3, 5], x[1, 0, 0], x[2, 1, 2] = -0.0, np.inf, np.nan
  x.view(np.int32)[0, 4, 4] = 1                                            # a denormal
  y, plan = aug_mod.apply_host(aug_mod.SpecAugment(aug_mod.IDENTITY, 5, [1, 2, 3]), x, [37, 20, 1])
  assert np.array_equal(np.ascontiguousarray(y).view(np.int32), x.view(np.int32))
  assert plan.tolist() == [[0, 0]] * 3
  assert aug_mod.IDENTITY.is_identity and not aug_mod.POLICIES['LB'].is_identity and aug_mod.POLICIES['LD'] == LD


def test_an_utterance_does_not_depend_on_its_batch():
  """Utterance u with draw id d: the same output at row 0 of a batch of 1 and at row 5 of a batch of 7 padded 300 frames longer."""
  aug_mod = A()
  rng = np.random.default_rng(8)
  L, C = 120, 80
  u = rng.standard_normal((L, C)).astype(np.float32)
  alone = np.zeros((1, L, C), dtype=np.float32)
  alone[0] = u
  crowd = rng.standard_normal((7, L + 300, C)).astype(np.float32)
  crowd[5, :L] = u
  policy = (10, 27, 2, 30, 2, 1.0)
  d = 123456789012
  y1, p1 = aug_mod.apply_host(aug_mod.SpecAugment(policy, 42, [d]), alone, [L])
  lens = [400, 33, 420, 1, 250, L, 77]
  y7, p7 = aug_mod.apply_host(aug_mod.SpecAugment(policy, 42, [5, 6, 7, 8, 9, d, 10]), crowd, lens)
  assert np.array_equal(p1[0], p7[5]) and p1[0, 0] > 0
  assert np.array_equal(np.ascontiguousarray(y1[0]).view(np.int32), np.ascontiguousarray(y7[5, :L]).view(np.int32))
  assert np.array_equal(np.ascontiguousarray(y7[5, L:]).view(np.int32), crowd[5, L:].view(np.int32))
  assert not np.array_equal(y1[0], u)


def test_draw_ids_of_ranks_are_the_global_batchs():
  aug_mod = A()
  for k in (0, 1, 7, 10 ** 9):
    whole = aug_mod.draw_ids(k, 6)
    assert whole.dtype == np.int64 and whole.tolist() == [k * 6 + r for r in range(6)]
    assert np.array_equal(np.concatenate([aug_mod.draw_ids(k, 3, world=2, rank=0), aug_mod.draw_ids(k, 3, world=2, rank=1)]), whole)
  aug = aug_mod.SpecAugment('LD', seed=-1)
  assert aug.seed == 2 ** 64 - 1 and aug.draw_ids is None
  assert aug.for_step(4, 3, world=2, rank=1).draw_ids.tolist() == [27, 28, 29] and aug.for_step(4, 3, 2, 1).policy == LD


def test_exports_and_argument_checks():
  from speecht_amd import _lib
  lib = _lib.load()
  header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'speecht_hip.h')).read(), flags=re.S)
  for name in ('st_spec_augment_f32', 'st_spec_augment_host', 'st_spec_augment_plan_host'):
    assert re.search(r'\b' + name + r'\s*\(', header) and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
  x = np.zeros((2, 8, 16), dtype=np.float32)
  out = np.zeros((2, 8, 16), dtype=np.float32)
  lens, ids = np.array([8, 3], dtype=np.int32), np.array([0, 1], dtype=np.int64)
  plan = np.zeros((2, 34), dtype=np.int32)
  p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
  dst = _lib.Tensor3(out.ctypes.data, 2, 8, 16, 0, 8, 16)
  good = dict(batch=2, frames=8, channels=16, W=2, F=3, mF=1, T=4, mT=1, q=65536)

  def host(lens=lens, dst=dst, **kw):
    a = dict(good, **kw)
    return lib.st_spec_augment_host(p(x), a['batch'], a['frames'], a['channels'], p(lens), p(ids), 7, a['W'], a['F'], a['mF'], a['T'], a['mT'],
                                    a['q'], ctypes.byref(dst), p(plan))

  def device(dst=dst, **kw):
    # (host pointers: every call below is refused before anything is launched or read)
    a = dict(good, **kw)
    return lib.st_spec_augment_f32(p(x), a['batch'], a['frames'], a['channels'], p(lens), p(ids), 7, a['W'], a['F'], a['mF'], a['T'], a['mT'],
                                   a['q'], ctypes.byref(dst), p(plan), None)

  def plans(lens=lens, **kw):
    a = dict(good, **kw)
    return lib.st_spec_augment_plan_host(p(lens), p(ids), a['batch'], a['channels'], 7, a['W'], a['F'], a['mF'], a['T'], a['mT'], a['q'], p(plan))
  assert host() == 0 and plans() == 0
  bad = [dict(batch=0), dict(channels=0), dict(mF=9), dict(mT=9), dict(mF=-1), dict(W=-1), dict(F=-1), dict(T=-1), dict(q=-1), dict(q=65537)]
  for kw in bad:
    assert host(**kw) == -1 and device(**kw) == -1 and plans(**kw) == -1, kw
    assert b'st_spec_augment' in lib.st_last_error()
  assert host(frames=0) == -1 and device(frames=0) == -1
  assert host(lens=np.array([9, 3], dtype=np.int32)) == -1 and b'length 9' in lib.st_last_error()       # L <= T
  assert host(lens=np.array([8, -1], dtype=np.int32)) == -1 and plans(lens=np.array([8, -1], dtype=np.int32)) == -1
  assert host(dst=_lib.Tensor3(out.ctypes.data, 2, 8, 16, 0, 7, 16)) == -1                                 # t_pitch < frames
  assert host(dst=_lib.Tensor3(out.ctypes.data, 2, 8, 12, 0, 8, 16)) == -1 and device(dst=_lib.Tensor3(out.ctypes.data, 2, 8, 12, 0, 8, 16)) == -1
  with pytest.raises(ValueError):
    A().SpecAugmentPolicy(1, 1, 9, 1, 1, 1.0)
  with pytest.raises(ValueError):
    A().SpecAugmentPolicy(1, 1, 1, 1, 1, 1.5)


def test_cli_flags_belong_to_train_alone(capsys):
  loader = importlib.machinery.SourceFileLoader('speecht_cli_spec_augment', os.path.join(ROOT, 'speecht-cli'))
  spec = importlib.util.spec_from_loader(loader.name, loader)
  cli = importlib.util.module_from_spec(spec)
  loader.exec_module(cli)
  aug_mod = A()
  _, flags = cli.parse(['train', '--spec-augment', 'LD', '--time-masks', '3'])
  aug = aug_mod.from_flags(flags)
  assert aug.policy == (80, 27, 2, 100, 3, 1.0) and aug.seed == 0
  _, flags = cli.parse(['train', '--spec-augment', 'LB', '--seed', '5', '--time-warp', '0', '--time-mask-ratio', '0.25', '--freq-mask-width', '15'])
  aug = aug_mod.from_flags(flags)
  assert aug.policy == (0, 15, 1, 100, 1, 0.25) and aug.seed == 5
  _, flags = cli.parse(['train', '--seed', '5', '--augment-seed', '9', '--time-warp', '40'])
  assert aug_mod.from_flags(flags).seed == 9 and aug_mod.from_flags(flags).policy == (40, 0, 0, 0, 0, 1.0)
  _, flags = cli.parse(['train'])
  assert flags.spec_augment == 'none' and aug_mod.from_flags(flags) is None
  for command in ('evaluate', 'search', 'export', 'preprocess'):
    with pytest.raises(SystemExit):
      cli.parse([command, '--spec-augment', 'LB'])
  capsys.readouterr()
  import speecht
  assert importlib.import_module('speecht.augmentation') is aug_mod and speecht.augmentation is aug_mod
