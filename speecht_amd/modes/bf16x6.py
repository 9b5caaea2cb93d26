"""bf16x6 mode (experimental, opt-in: ST_CONV_MODE=bf16x6): the layers that stay GEMMs -- at the training shapes the 2000 x 2000
layer -- as fp32-accurate products of three exact bf16 pieces per operand, six terms on the bf16 matrix pipe with fp32
accumulation (csrc/conv_bf16.hip, NP = 3); everything else as in the fp32 mode it derives from."""
import torch

from .._lib import call
from ..engine_buffers import _round_up
from .fp32 import Fp32Mode


class Bf16x6Mode(Fp32Mode):
  _one_tap_in_place = False
  _flip_every_layer = True
  _top_gradient_beside = False
  masks_padding = False             # (its plane plumbing hands operands from layer to layer beside the time-domain rows)
  cache_shapes = False              # (its weight planes are re-chosen per shape in `_alloc_planes`: described anew every time)

  def __init__(self, engine):
    super().__init__(engine)
    # three-piece planes of the weights / of their flipped copies: the buffers by layer (kept across shapes), the ones of the
    # layers on this path for the current shape, and whether those follow the weights
    self._wp_store, self._wtp_store, self.Wp, self.WTp = {}, {}, {}, {}
    self._wplanes_fresh = self._wtplanes_fresh = False

  def weights_changed(self):
    super().weights_changed()
    self._wplanes_fresh = self._wtplanes_fresh = False

  def _refresh_backward_operands(self):
    super()._refresh_backward_operands()
    self._wtplanes_fresh = False                   # (split from the copies just rebuilt)

  def _workspace_bytes(self, lib, sh):
    ws = super()._workspace_bytes(lib, sh)
    return max([ws] + [lib.st_exp_conv1d_bwd_data_bf16x6_ws(sh.dZ[i].ref, sh.dZ[i - 1].ref, l.width) for i, l in enumerate(self.e.layers) if i > 0])

  def prepare_forward_graph(self):
    if not self._wplanes_fresh:
      self._refresh_wplanes()
    super().prepare_forward_graph()

  # ---- which layers take the bf16x6 kernels ------------------------------------------------------------------------
  def _in_fft(self, part, i):
    return self.e.fft_conv and i in part.fft_layers

  def _x6_fwd(self, part, i):
    return self.e.layers[i].n_pad % 128 == 0 and not self._in_fft(part, i)

  def _x6_bwd(self, part, i):
    l = self.e.layers[i]
    return (i > 0 and l.nt_pad % 128 == 0 and l.width * l.cout_pitch >= 256 and not self._in_fft(part, i))

  def _x6_wgrad(self, part, i):
    l = self.e.layers[i]
    tiles = -(-(l.width * l.cin_pitch) // 128) * (l.n_pad // 128)
    return (i > 0 and l.stride == 1 and l.n_pad % 128 == 0 and tiles >= 192 and not self._in_fft(part, i))

  def _alloc_planes(self, sh, part):
    """The part's planes of the activations on this path (Xp, dZp, tq, XTp, dZTp) and the mode's weight planes."""
    e, X, dZ, layers = self.e, sh.X, sh.dZ, self.e.layers
    planes = lambda name, numel: e._planes(sh.ranges, name, numel)
    part.Xp = {i: planes('Xp%d' % i, X[i].buf.numel()) for i in range(len(layers)) if self._x6_fwd(part, i)}
    part.dZp = {i: planes('dZp%d' % i, dZ[i].buf.numel()) for i in range(len(layers)) if self._x6_bwd(part, i)}
    # filter gradient: transposed (reduction-major) planes of the layer input and of dz
    part.tq, part.XTp, part.dZTp = {}, {}, {}
    for i, l in enumerate(layers):
      if self._x6_wgrad(part, i):
        tq = _round_up(max(X[i].t_pitch, dZ[i].frames), 32)
        red = X[i].batch * tq
        part.tq[i] = tq
        part.XTp[i] = planes('XTp%d' % i, l.cin_pitch * red + 4096)
        part.dZTp[i] = planes('dZTp%d' % i, l.n_pad * red)
    # weight planes of exactly the layers that run on this path for the current shape (the frequency-domain set
    # depends on the shape); buffers are kept across shapes
    def kept(store, i, numel):
      if i not in store:
        store[i] = torch.zeros(numel, dtype=torch.bfloat16, device=e.device)
      return store[i]
    self.Wp = {i: kept(self._wp_store, i, 3 * l.k_pad * l.n_pad) for i, l in enumerate(layers) if self._x6_fwd(part, i)}
    self.WTp = {i: kept(self._wtp_store, i, 3 * l.kt_pad * l.nt_pad) for i, l in enumerate(layers) if self._x6_bwd(part, i)}
    self._wplanes_fresh = False
    self._wtplanes_fresh = False

  def _refresh_wplanes(self):
    e = self.e
    for i, wp in self.Wp.items():
      l = e.layers[i]
      pf, _ = e._slice(e.params, i)
      call('st_exp_split3_transpose_bf16', e._ptr(pf), l.k_pad, l.n_pad, e._ptr(wp), e.stream_ptr)
    self._wplanes_fresh = True

  def _refresh_wtplanes(self):
    e = self.e
    for i, wp in self.WTp.items():
      l = e.layers[i]
      call('st_exp_split3_transpose_bf16', e._ptr(e.packed_t[i]), l.kt_pad, l.nt_pad, e._ptr(wp), e.stream_ptr)
    self._wtplanes_fresh = True

  # ---- the per-layer hooks of Fp32Mode.forward / backward ------------------------------------------------------------
  def _forward_prologue(self):
    e, sh = self.e, self.e.shape
    if not self._wplanes_fresh:
      self._refresh_wplanes()
    if self._x6_fwd(sh.mode, 0):
      call('st_exp_split3_bf16', e._ptr(sh.X[0].buf), sh.X[0].buf.numel(), e._ptr(sh.mode.Xp[0]), e.stream_ptr)

  def _x6_forward_layer(self, i, pb):
    e, ptr = self.e, self.e._ptr
    sh, l, s = e.shape, e.layers[i], e.stream_ptr
    X, part = sh.X, sh.mode
    if i > 0 and not self._x6_fwd(part, i - 1):
      call('st_exp_split3_bf16', ptr(X[i].buf), X[i].buf.numel(), ptr(part.Xp[i]), s)
    yp = ptr(part.Xp[i + 1]) if (i + 1 < len(e.layers) and self._x6_fwd(part, i + 1)) else None
    call('st_exp_conv1d_fwd_bf16x6', X[i].ref, ptr(part.Xp[i]), ptr(self.Wp[i]), ptr(pb), l.width, l.stride, sh.geo[i][2],
         int(l.relu), X[i + 1].ref, yp, s)

  def _backward_prologue(self):
    self._wait_bwd_operands()                   # the split planes are derived from all transposed copies at once

  def _x6_filter_gradient(self, i, gf, gb, need_bias):
    e, ptr = self.e, self.e._ptr
    sh, l, s = e.shape, e.layers[i], e.stream_ptr
    x, dz, part = sh.X[i], sh.dZ[i], sh.mode
    tq, red = part.tq[i], x.batch * part.tq[i]
    call('st_exp_transpose_split3_bf16', x.ref, 0, x.t_pitch, tq, l.cin_pitch * red + 4096, ptr(part.XTp[i]), s)
    call('st_exp_transpose_split3_bf16', dz.ref, dz.halo, dz.frames, tq, l.n_pad * red, ptr(part.dZTp[i]), s)
    call('st_exp_conv1d_bwd_filter_bf16x6', ptr(part.XTp[i]), ptr(part.dZTp[i]), x.batch, tq, l.width, l.cin_pitch,
         x.halo - sh.geo[i][2], l.cout, ptr(gf), s)
    if need_bias:
      call('st_bias_grad_f32', dz.ref, ptr(gb), ptr(part.wgrad_ws), part.wgrad_ws.numel() * 4, s)

  def _x6_back_prop(self, i):
    e, ptr = self.e, self.e._ptr
    sh, l, s = e.shape, e.layers[i], e.stream_ptr
    X, dZ, part = sh.X, sh.dZ, sh.mode
    act = X[i].ref if e.layers[i - 1].relu else None
    if not self._wtplanes_fresh:
      self._refresh_wtplanes()
    if not (i + 1 < len(e.layers) and self._x6_bwd(part, i + 1)):       # producer was not on this path
      call('st_exp_split3_bf16', ptr(dZ[i].buf), dZ[i].buf.numel(), ptr(part.dZp[i]), s)
    dxp = ptr(part.dZp[i - 1]) if self._x6_bwd(part, i - 1) else None
    call('st_exp_conv1d_bwd_data_bf16x6', dZ[i].ref, ptr(part.dZp[i]), ptr(self.WTp[i]), l.width, sh.geo[i][2], act, dZ[i - 1].ref,
         dxp, ptr(part.wgrad_ws), part.wgrad_ws.numel() * 4, s)
