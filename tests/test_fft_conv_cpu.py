"""The frequency-domain layers without a GPU: the float64 reference for a convolution with any left padding
(tests/conv_pad_ref.py) against the oracle, and the argument checks of the C ABI in csrc/conv_fft.hip -- all made before any
launch -- for the range of filter widths: a window of N = 63 + W frames needs N / 2 + 1 bins and the spectrum matrices have
48 rows, so 32 taps (N = 95, 48 bins) is the widest layer; 33 taps (N = 96) would need a 49th."""
import ctypes

import numpy as np
import pytest

from oracle import w2l_oracle as O
from tests.conv_pad_ref import conv1d_pad_bwd, conv1d_pad_fwd


@pytest.mark.parametrize('W,T', [(2, 5), (7, 70), (8, 9), (32, 3), (33, 40)])
@pytest.mark.parametrize('relu', [True, False])
def test_padded_reference_is_the_oracle_at_the_same_padding(W, T, relu):
  rng = np.random.default_rng(W * 100 + T)
  x = rng.standard_normal((2, T, 5))
  F = rng.standard_normal((W, 5, 6))
  bias = rng.standard_normal(6)
  pl = O.same_padding(T, W, 1)[1]
  y = conv1d_pad_fwd(x, F, bias, pl, relu)
  y_ref = O.conv1d_same_fwd(x, F, bias, 1, relu)
  np.testing.assert_allclose(y, y_ref, rtol=0, atol=1e-12 * np.max(np.abs(y_ref)))
  dy = rng.standard_normal(y.shape)
  refs = O.conv1d_same_bwd(x, F, y_ref, dy, 1, relu)
  outs = conv1d_pad_bwd(x, F, dy * (y_ref > 0) if relu else dy, pl)
  for a, b in zip(outs, refs):
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-12 * np.max(np.abs(b)))


def test_padded_reference_moves_with_the_left_padding():
  # one tap of weight 1 at w = 2 of 4, an impulse at t = 3: y[t] = x[t + 2 - pl]
  x = np.zeros((1, 8, 1))
  x[0, 3, 0] = 1.0
  F = np.zeros((4, 1, 1))
  F[2] = 1.0
  for pl in range(4):
    y = conv1d_pad_fwd(x, F, np.zeros(1), pl, relu=False)
    assert np.argmax(y[0, :, 0]) == 3 - 2 + pl and y.sum() == 1.0


def _lib_and_tensor():
  from speecht_amd import _lib
  from speecht_amd._lib import Tensor3
  lib = _lib.load()
  host = (ctypes.c_float * 16)()                                   # never dereferenced: the sizing functions read the descriptor only
  t = Tensor3(ctypes.addressof(host), 3, 130, 100, 16, 130 + 32, 112)
  return _lib, lib, t


def test_a_33_tap_layer_is_refused_before_any_launch():
  _lib, lib, t = _lib_and_tensor()
  with pytest.raises(_lib.SpeechtHipError, match=r'filter width must be in \[2, 32\]'):
    _lib.call('st_conv1d_fft_plan', 33, 130, 3, None, None, None, None, None)
  assert lib.st_conv1d_fft_filter_floats(33, 112, 128) == 0
  assert lib.st_conv1d_fft_sf_floats(ctypes.byref(t), ctypes.byref(t), 33) == 0
  assert lib.st_conv1d_fft_zf_floats(ctypes.byref(t), 33) == 0
  assert lib.st_conv1d_fft_ws(ctypes.byref(t), ctypes.byref(t), 33) == 0
  tables = (ctypes.c_float * lib.st_conv1d_fft_table_floats())()
  with pytest.raises(_lib.SpeechtHipError, match='fft tables: bad argument'):
    _lib.call('st_conv1d_fft_tables_f32', 33, 16, ctypes.cast(tables, ctypes.c_void_p), len(tables), None)
  assert not any(tables)


@pytest.mark.parametrize('W,n,bins', [(32, 95, 48), (2, 65, 33)])
def test_the_ends_of_the_width_range_are_planned(W, n, bins):
  _lib, lib, t = _lib_and_tensor()
  got = [ctypes.c_int() for _ in range(5)]
  _lib.call('st_conv1d_fft_plan', W, 130, 3, *[ctypes.byref(g) for g in got])
  assert [g.value for g in got] == [n, 64, 3, bins, 128]            # n, frames per block, blocks, bins, rows per bin (9 -> 128)
  assert lib.st_conv1d_fft_filter_floats(W, 112, 128) == bins * 2 * 128 * 2 * 128
  assert lib.st_conv1d_fft_sf_floats(ctypes.byref(t), ctypes.byref(t), W) == bins * 2 * 128 * 2 * 128
  assert lib.st_conv1d_fft_zf_floats(ctypes.byref(t), W) == bins * 128 * 2 * 128
  with pytest.raises(_lib.SpeechtHipError):
    _lib.call('st_conv1d_fft_plan', 1 if W == 2 else 33, 130, 3, None, None, None, None, None)
