"""Float64 stride-1 convolution with ANY left padding: y[t] = sum_w F[w] x[t + w - pl] + bias, zeros outside the input, and its
three gradients.  With pl the SAME padding it is oracle.conv1d_same_fwd / conv1d_same_bwd (tests/test_fft_conv_cpu.py); the
frequency-domain entry points (csrc/conv_fft.hip) admit every pl in [0, W), which the oracle does not express."""
import numpy as np


def _windows(x, W, pl):
  T = x.shape[1]
  xp = np.pad(x, ((0, 0), (pl, W - 1 - pl), (0, 0)))
  return np.stack([xp[:, w:w + T] for w in range(W)], axis=2)          # [B, T, W, Cin]


def conv1d_pad_fwd(x, F, bias, pl, relu=True):
  y = np.einsum('btwc,wco->bto', _windows(x, F.shape[0], pl), F) + bias
  return np.maximum(y, 0.0) if relu else y


def conv1d_pad_bwd(x, F, dz, pl):
  """dz: gradient wrt the pre-activation output.  Returns (dx, dF, db)."""
  W, T = F.shape[0], x.shape[1]
  dF = np.einsum('btwc,bto->wco', _windows(x, W, pl), dz)
  dcols = np.einsum('bto,wco->btwc', dz, F)
  dxp = np.zeros((x.shape[0], T + W - 1, x.shape[2]))
  for w in range(W):
    dxp[:, w:w + T] += dcols[:, :, w]
  return dxp[:, pl:pl + T], dF, dz.sum(axis=(0, 1))
