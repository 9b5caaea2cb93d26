"""fp32 mode (BASELINE configs[1], the headline): exact-fp32 MFMA kernels (csrc/conv_gemm.hip) with nine of the eleven
layers in the frequency domain (csrc/conv_fft.hip, `SpectralLayers`).  The bf16x6 mode derives from this class and
overrides the per-layer hooks `_x6_*`."""
import ctypes
import os
from types import SimpleNamespace

import torch

from .. import _lib
from .._lib import call
from .base import ModeBase
from .spectral import SpectralLayers


class Fp32Mode(SpectralLayers, ModeBase):
  _one_tap_in_place = True        # 1-tap layers back-propagate through their own packed filters read transposed
  _flip_every_layer = False       # (bf16x6: every layer's operand planes are split from a flipped / transposed copy)
  masks_padding = True

  def __init__(self, engine):
    super().__init__(engine)
    # the flipped / transposed weight copies (`engine.packed_t`): current? for which layers? events of a rebuild on the side stream
    self._packed_t_fresh, self._packed_t_layers, self._bwd_ready = False, frozenset(), {}
    # the frequency-domain layers across shapes (SpectralLayers)
    self._gfwd_fresh, self._gfwd_ready, self._fft_table_key, self._fft_prev = False, {}, {}, None

  def weights_changed(self):
    self._packed_t_fresh = False
    self._gfwd_fresh = False

  def forget_tables(self):
    self._fft_table_key = {}

  # ---- buffers ---------------------------------------------------------------------------------------------------
  def alloc(self, sh):
    """-> the part of `sh` this mode reads: wgrad_ws, wgrad_ws_top, side_wgrad_top, fft_layers, fft, table_keys (bf16x6: + planes)."""
    lib, e, part = _lib.load(), self.e, SimpleNamespace()
    ws = self._workspace_bytes(lib, sh)
    part.wgrad_ws, _ = e._storage.view('wgrad_ws', ws // 4 + 64)
    # The classification layer (2000 -> 29): its filter gradient streams the activations, its back-prop to the input streams
    # the mask and writes dZ of the layer below -- two HBM-bound launches of ~90 us each that do not depend on each other.
    # Side by side on two streams (own scratch for the one on the side stream).
    top = len(e.layers) - 1
    part.side_wgrad_top = (self._top_gradient_beside and e.side_filter_gradient and os.environ.get('ST_WGRAD_SIDE_TOP', '1') != '0' and
                           top > 0 and e.layers[top].cout <= 64 and e.layers[top].width == 1)
    part.wgrad_ws_top = None
    if part.side_wgrad_top:
      ws_top = lib.st_conv1d_bwd_filter_ws(sh.X[top].ref, sh.dZ[top].ref, e.layers[top].width)
      part.wgrad_ws_top, _ = e._storage.view('wgrad_ws_top', ws_top // 4 + 64)
    # which layers run in the frequency domain is decided first: they leave the bf16x6 plane plumbing alone
    part.fft_layers = {i for i in range(len(e.layers)) if self._use_fft(i, sh.batch, sh.geo)}
    self._alloc_planes(sh, part)
    self._alloc_fft(sh, part)
    return part

  _top_gradient_beside = True

  def reenter(self, sh):
    self._fft_transition(sh.mode.fft, sh.mode.table_keys)

  def _workspace_bytes(self, lib, sh):
    layers, X, dZ = self.e.layers, sh.X, sh.dZ
    ws = max(lib.st_conv1d_bwd_filter_ws(X[i].ref, dZ[i].ref, l.width) for i, l in enumerate(layers))
    ws = max([ws] + [lib.st_conv1d_bwd_data_bias_ws(dZ[i].ref, dZ[i - 1].ref, l.width) for i, l in enumerate(layers) if i > 0])
    return max([ws] + [lib.st_conv1d_fwd_ws(X[i].ref, X[i + 1].ref, l.width) for i, l in enumerate(layers)])

  # ---- hooks of the bf16x6 mode (nothing here) -----------------------------------------------------------------------
  # (`_x6_forward_layer`, `_x6_filter_gradient`, `_x6_back_prop` are reached only where these hold: Bf16x6Mode has them)
  def _x6_fwd(self, part, i):
    return False
  _x6_bwd = _x6_wgrad = _x6_fwd

  def _alloc_planes(self, sh, part):
    pass

  def _forward_prologue(self):
    pass
  _backward_prologue = _forward_prologue

  # ---- refreshes -----------------------------------------------------------------------------------------------------
  def refresh_under_ctc(self):
    # the filter operands of back-prop (flipped / transposed copies of the weights Adam just updated) are rebuilt
    # on the side stream while the CTC recursion runs
    if not self._packed_t_ok() and self._flip_layers():
      self.e._on_side_stream(self._refresh_backward_operands)

  def prepare_forward_graph(self):
    e = self.e
    e._join_side_stream()
    if e.shape.mode.fft and e.fft_conv and not self._gfwd_fresh:
      self._refresh_fft_filters()
    self._wait_gfwd()                              # no waits on outside events inside a capture

  def _transposed_in_place(self, i):
    """Back-prop to the input of layer i reads the layer's own packed filters as a transposed operand
    (st_conv1d_1tap_bwd_data_bias_f32): one tap, whole 32-deep k-tiles over the output channels."""
    l = self.e.layers[i]
    return (self._one_tap_in_place and i > 0 and l.width == 1 and l.stride == 1 and l.cout_pitch % 32 == 0 and
            l.n_pad >= l.cout_pitch and l.nt_pad % 128 == 0)

  def _flip_layers(self):
    """Layers whose back-prop to the input still needs the flipped / transposed copy of the weights: W-tap layers of
    more than one tap (and everything on the bf16x6 path, whose operand planes are split from those copies).  The
    frequency-domain layers read their forward spectra transposed, 1-tap layers their packed filters (round 4): at the
    model's training shapes NO copy is rebuilt any more (rounds 1-3: ~0.33 ms of HBM-bound launches per step)."""
    e = self.e
    fft = e.shape.mode.fft if e.fft_conv else ()
    return [i for i in range(1, len(e.layers)) if self._flip_every_layer or not (i in fft or self._transposed_in_place(i))]

  def _refresh_backward_operands(self):
    """The flipped / transposed weight copies of the layers that still need one (`_flip_layers`), top layer first, the order
    back-prop consumes them in; an event after each lets the compute stream wait for what it is about to use only."""
    e, ptr, s, stream, flip = self.e, self.e._ptr, self.e.stream_ptr, self.e.stream, self._flip_layers()
    self._bwd_ready = {}
    for i in reversed(flip):
      l = e.layers[i]
      call('st_filters_flip_transpose_f32', ptr(e._slice(e.params, i)[0]), l.width, l.cin, l.cout, l.cin_pitch, l.cout_pitch,
           ptr(e.packed_t[i]), s)
      ev = torch.cuda.Event()
      ev.record(stream)
      self._bwd_ready[i] = ev
    self._packed_t_fresh = True
    self._packed_t_layers = frozenset(flip)

  def _packed_t_ok(self):
    """The flipped / transposed copies are current for every layer that needs one NOW: which layers do depends on state that
    can change between steps (the shape's frequency-domain set, `fft_conv`), so a refresh remembers the set it rebuilt."""
    return self._packed_t_fresh and frozenset(self._flip_layers()) <= self._packed_t_layers

  def _wait_bwd_operands(self, i=None):
    """The compute stream waits for the back-prop operands of layer i (None: of every layer) if they were rebuilt on the
    side stream.  The side stream works top layer first, so a lower layer's event covers the ones above it."""
    ready = self._bwd_ready
    if not ready:
      return
    keys = [k for k in ready if i is None or k >= i]
    if keys:
      self.e.stream.wait_event(ready[min(keys)])
      for k in keys:
        del ready[k]

  def forward(self, mask_padding=False):
    """X[0] -> logits X[-1] through the eleven layers (speech_model.py:279-295): per layer the frequency-domain entry
    point, the W-tap kernel or -- in the bf16x6 mode -- that mode's kernel, as decided per shape by `_use_fft` / `_x6_fwd`.
    ``mask_padding``: every layer's output but the last is masked in the time domain (st_mask_rows), so a frequency-domain layer
    never hands input spectra to the next one -- they would be the spectra of the unmasked rows."""
    if mask_padding and not self.masks_padding:
      raise _lib.SpeechtHipError('forward(mask_padding=True) is not supported by this mode')
    e, ptr, sh, s = self.e, self.e._ptr, self.e.shape, self.e.stream_ptr
    valid, top = (e._mask_lengths(), len(e.layers) - 1) if mask_padding else (None, 0)
    X, geo, part = sh.X, sh.geo, sh.mode
    fft = part.fft if e.fft_conv else {}                   # the layers that run in the frequency domain now
    ws = part.wgrad_ws
    ws_bytes = ws.numel() * 4 if e.split_small_batches else 0
    self._forward_prologue()
    sf_ready = False                 # the previous layer's call left this layer's input spectra behind
    for i, l in enumerate(e.layers):
      pf, pb = e._slice(e.params, i)
      if i not in fft:
        sf_ready = False
      if self._x6_fwd(part, i):
        self._x6_forward_layer(i, pb)
      elif i in fft:
        f = fft[i]
        if not self._gfwd_fresh:
          e._join_side_stream()
          self._refresh_fft_filters()
        self._wait_gfwd(i)                               # the filter spectra may still be on their way (side stream)
        # a chain of frequency-domain layers: where the shapes allow, this layer's inverse transform hands its frames to the
        # next layer's forward transform in registers and leaves that layer's input spectra behind (`sf_ready` for its call)
        nxt = None if mask_padding else fft.get(i + 1)
        if nxt is not None and nxt['shift'] is not None:
          nxt = None
        written = ctypes.c_int(0)
        call('st_conv1d_nwc_fwd_fft_chain_f32', f['xref'], ptr(f['gfwd']), ptr(pb), f['width'], f['pl'], int(l.relu), X[i + 1].ref,
             ptr(f['tables']), ptr(f['sf']), int(sf_ready), ptr(nxt['tables']) if nxt else None, ptr(nxt['sf']) if nxt else None,
             nxt['width'] if nxt else 0, nxt['pl'] if nxt else 0, ctypes.byref(written), ptr(f['ws']), f['ws'].numel() * 4, s)
        sf_ready = written.value == 1
      else:
        call('st_conv1d_nwc_fwd_ws_f32', X[i].ref, ptr(pf), ptr(pb), l.width, l.stride, geo[i][2], int(l.relu), X[i + 1].ref,
             ptr(ws), ws_bytes, s)
      if mask_padding and i < top:
        call('st_mask_rows', X[i + 1].ref, valid(i), 4, s)

  def backward(self, on_layer_done, wanted):
    """Back-prop from dZ[-1] through the frequency-domain / W-tap (/ bf16x6) kernels; hooks as `Wav2LetterEngine.backward`
    describes them."""
    e, ptr, sh, s, layers = self.e, self.e._ptr, self.e.shape, self.e.stream_ptr, self.e.layers
    X, dZ, geo, part = sh.X, sh.dZ, sh.geo, sh.mode
    fft = part.fft if e.fft_conv else {}                   # the layers that run in the frequency domain now
    wgrad_ws, wgrad_ws_bytes = part.wgrad_ws, part.wgrad_ws.numel() * 4
    if not self._packed_t_ok():
      self._refresh_backward_operands()           # (normally done on the side stream by ctc_loss_grad; nothing at the model's shapes)
    if fft and not self._gfwd_fresh:
      e._join_side_stream()                         # (weights written after the forward pass: back-prop reads the same spectra)
      self._refresh_fft_filters()
    self._wait_gfwd()
    self._backward_prologue()
    # waits per layer; after the two layers on top one wait covers everything below (by then the side stream is through)
    wait_all_below = len(layers) - 3
    side_wgrad, deferred = False, None     # a filter gradient is in flight on the side stream; its layer's hook is due
    top_pending = None                     # the classification layer's filter gradient is in flight on the second side stream
    hook = on_layer_done
    if hook is not None:
      def on_layer_done(j):
        nonlocal top_pending
        if top_pending is not None and top_pending != j:
          e._join_side_stream(second_only=True)
          hook(top_pending)
          top_pending = None
        if top_pending != j:
          hook(j)
    bias_from_above = False      # layer i's bias gradient already written by the back-prop kernel of layer i + 1
    zf_ready = False             # layer i's dz spectra already written by the back-prop kernel of layer i + 1
    for i in reversed(range(len(layers))):
      l = layers[i]
      gf, gb = e._slice(e.grads, i)
      need_bias, bias_from_above = not bias_from_above, False
      if self._x6_wgrad(part, i):
        self._x6_filter_gradient(i, gf, gb, need_bias)
      elif i in fft:
        f = fft[i]
        # the spectra of dz serve the filter gradient here and back-prop to the input below (the layer above may have left
        # them behind already: its back-prop kernel transformed the frames it had just produced, `zf_ready`)
        if not zf_ready:
          call('st_conv1d_fft_dz_spectra_f32', dZ[i].ref, f['width'], ptr(f['tables']), ptr(f['zf']), s)
        zf_ready = False
        polyphase = f['shift'] is not None       # the gradient comes out in the shifted layout of the polyphase taps

        # (run now or on a side stream: `e.stream` / `e.stream_ptr` are read when it runs)
        def filter_gradient(f=f, l=l, i=i, gf=gf, gb=gb, need_bias=need_bias, polyphase=polyphase, ws=f.get('ws2', f['ws'])):
          call('st_conv1d_nwc_bwd_filter_fft_f32', f['xref'], dZ[i].ref, ptr(f['sf']), ptr(f['zf']), f['width'], ptr(f['tables']),
               ptr(f['dpacked2'] if polyphase else gf), ptr(ws), ws.numel() * 4, e.stream_ptr)
          if polyphase:
            cp = X[i].c_pitch
            n, o = l.width * cp * l.n_pad, f['shift'] * cp * l.n_pad
            with torch.cuda.stream(e.stream):
              gf[:n].copy_(f['dpacked2'][o:o + n], non_blocking=True)
          if need_bias:      # bin 0 of the spectra is the sum over the frames
            call('st_conv1d_fft_bias_grad_f32', dZ[i].ref, f['width'], ptr(f['zf']), ptr(gb), e.stream_ptr)
        if 'ws2' in f:
          # The filter gradient (lag products, inverse transform of the filters, bias sum) and back-prop to the input
          # (products, inverse transform) both hang off the spectra of dz and are independent: on two streams.  The
          # narrow layers' products (36 bins x 16 tiles) leave a quarter of the CU slots of their last round empty --
          # side by side they fill each other's gaps -- and the HBM-bound transforms of one chain run under the
          # matrix-pipe-bound products of the other (measured: 7.84 -> 7.43 ms per step).
          # (round 4: with back-prop's transforms fused the compute stream needs ~80 us per narrow layer, ONE side stream's
          # chain -- 73 + 42 + 9 us, in order -- had become the pace of the backward pass: the chains take the two side streams in turn)
          e._on_side_stream(filter_gradient, second=(i % 2 == 1))
          side_wgrad, deferred = True, i
        else:
          filter_gradient()
      elif i + 1 == len(layers) and part.side_wgrad_top:
        def top_gradient(i=i, l=l, gf=gf, gb=gb, need_bias=need_bias, ws=part.wgrad_ws_top):
          call('st_conv1d_nwc_bwd_filter_f32', X[i].ref, dZ[i].ref, l.width, l.stride, geo[i][2], ptr(gf),
               ptr(gb) if need_bias else None, ptr(ws), ws.numel() * 4, e.stream_ptr)
        # on the SECOND side stream (the first is still rebuilding back-prop operands when CTC ends); its hook is due with
        # the next layer's -- the two share a reduce bucket, and nothing waits for this launch until then
        e._on_side_stream(top_gradient, second=True)
        top_pending = i
      else:
        call('st_conv1d_nwc_bwd_filter_f32', X[i].ref, dZ[i].ref, l.width, l.stride, geo[i][2], ptr(gf),
             ptr(gb) if need_bias else None, ptr(wgrad_ws), wgrad_ws_bytes, s)
      if on_layer_done is not None and deferred != i and wanted(i):
        if side_wgrad:
          # this layer's own gradient ran on the compute stream, but its bucket also holds the layers above whose filter
          # gradients are still in flight on the side streams (the bottom bucket L0..L3: L1-L3 went there, L0 did not): the
          # exchange is ordered behind the compute stream only, so the compute stream waits for them first
          e._join_side_stream()
          side_wgrad = False
        on_layer_done(i)
      if i > 0 and self._x6_bwd(part, i):
        self._x6_back_prop(i)
      elif i > 0 and i in fft:
        f = fft[i]
        act = X[i].ref if layers[i - 1].relu else None
        below = part.fft.get(i - 1)                  # a frequency-domain layer below: its dz spectra can ride along
        written = ctypes.c_int(0)
        call('st_conv1d_nwc_bwd_data_fft_chain_f32', dZ[i].ref, ptr(f['zf']), ptr(f['gfwd']), l.width, geo[i][2], act,
             dZ[i - 1].ref, ptr(f['tables']), ptr(below['tables']) if below else None, ptr(below['zf']) if below else None,
             below['width'] if below else 0, ctypes.byref(written), ptr(f['ws']), f['ws'].numel() * 4, s)
        zf_ready = written.value == 1
      elif i > 0:
        # X[i] is the ReLU output of layer i-1: its sign is the mask of tf.nn.relu's gradient
        # the kernel that writes dZ[i-1] also sums its columns: the bias gradient of layer i - 1
        act = X[i].ref if layers[i - 1].relu else None
        if self._transposed_in_place(i):           # dx = dz W^T straight from the layer's packed filters
          call('st_conv1d_1tap_bwd_data_bias_f32', dZ[i].ref, ptr(e._slice(e.params, i)[0]), act, dZ[i - 1].ref,
               ptr(e._slice(e.grads, i - 1)[1]), ptr(wgrad_ws), wgrad_ws_bytes, s)
        else:
          self._wait_bwd_operands(i if i > wait_all_below else None)
          call('st_conv1d_nwc_bwd_data_bias_f32', dZ[i].ref, ptr(e.packed_t[i]), l.width, geo[i][2], act, dZ[i - 1].ref,
               ptr(e._slice(e.grads, i - 1)[1]), ptr(wgrad_ws), wgrad_ws_bytes, s)
        bias_from_above = True
      if deferred == i and on_layer_done is not None and wanted(i):
        # the gradient of this layer is complete when the side stream is (and with it those of the layers above that went
        # the same way: the stream runs in order): hand the bucket to the all-reduce only now, with back-prop to the input
        # already enqueued beside it
        e._join_side_stream()
        side_wgrad = False
        on_layer_done(i)
      if deferred == i:
        deferred = None
    if side_wgrad or top_pending is not None:
      e._join_side_stream()
    if top_pending is not None and hook is not None:
      hook(top_pending)
