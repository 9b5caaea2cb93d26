"""bf16 activations (BASELINE configs[3] arithmetic; csrc/conv_bf16.hip NP = 1, csrc/wgrad_tr_bf16.hip, the 32-tap layer through
st_conv1d_*_fft_planes): activations and activation gradients in HBM as bf16, fp32 masters / accumulation / logits / CTC / Adam."""
import ctypes
import os
from types import SimpleNamespace

import torch

from .. import _lib
from .._lib import call
from .base import ModeBase


class Bf16Mode(ModeBase):
  masks_padding = True

  def __init__(self, engine):
    super().__init__(engine)
    self.Wb = self.WTb = None                      # bf16 copies of the filters / of their flipped transposes (made by the first `alloc`)
    self._wplanes_fresh = self._wtplanes_fresh = False       # ... and whether they (and the filter spectra) follow the weights
    self._wb_ready, self._wb_order = {}, []        # events of a rebuild of `Wb` on the side stream, and the order it works in
    self._fftb_table_key, self._fftb_prev = {}, None         # as SpectralLayers' `_fft_table_key`, `_fft_prev`

  def weights_changed(self):
    self._wplanes_fresh = self._wtplanes_fresh = False

  def forget_tables(self):
    self._fftb_table_key = {}

  def alloc(self, sh):
    """-> the part of `sh` this mode reads: the bf16 planes Xb / dZb, which filter-gradient kernel each layer takes (_wgrad_tr) and
    on which stream (_side_wgrad_bf16), scratch (wgrad_ws_b, _b2, _b3), the frequency-domain layers (fftb_layers, fftb, table_keys)."""
    lib, e, ptr, part = _lib.load(), self.e, self.e._ptr, SimpleNamespace()
    X, dZ, geo, batch, layers, L = sh.X, sh.dZ, sh.geo, sh.batch, e.layers, len(e.layers)
    # the wide long-filter layer in the frequency domain with its per-bin products on the bf16 matrix pipe
    part.fftb_layers = {i for i in range(L) if self._use_fft_bf16(i, batch, geo[i][1])}
    # the filter gradients of the stride-1 layers read both planes as they lie (LDS transpose reads, csrc/wgrad_tr_bf16.hip) and
    # run up to `slack` rows past the last one: zeros behind every plane
    slack = lib.st_conv1d_bwd_filter_tr_bf16_slack_rows()
    part.Xb = [e._planes(sh.ranges, 'Xb%d' % i, X[i].buf.numel(), 1, slack * X[i].c_pitch) for i in range(L)]
    part.dZb = [e._planes(sh.ranges, 'dZb%d' % i, dZ[i].buf.numel(), 1, slack * dZ[i].c_pitch) for i in range(L)]
    part._wgrad_tr = [os.environ.get('ST_BF16_WGRAD_TR', '1') != '0' and
                      lib.st_conv1d_bwd_filter_tr_bf16_ws(X[i].ref, dZ[i].ref, l.width, l.stride, geo[i][2]) > 0
                      for i, l in enumerate(layers)]
    wgrad_ws = lambda i: (lib.st_conv1d_bwd_filter_tr_bf16_ws if part._wgrad_tr[i] else lib.st_conv1d_bwd_filter_bf16_ws)(
        X[i].ref, dZ[i].ref, layers[i].width, layers[i].stride, geo[i][2])
    ws = max(wgrad_ws(i) for i in range(L))
    ws = max([ws] + [lib.st_conv1d_bwd_data_bf16_ws(dZ[i].ref, dZ[i - 1].ref, l.width) for i, l in enumerate(layers) if i > 0])
    ws = max([ws] + [lib.st_conv1d_fwd_bf16_ws(X[i].ref, X[i + 1].ref, l.width) for i, l in enumerate(layers)])
    part.wgrad_ws_b, _ = e._storage.view('wgrad_ws_b', ws // 4 + 64)
    # the narrow layers' filter gradients run beside back-prop to the input on the side stream: their own scratch
    # (the classification layer beside its back-prop, as in fp32: measured, no gain here -- 3.15 ms either way)
    part._side_wgrad_bf16 = [i for i, l in enumerate(layers) if e.side_filter_gradient and i > 0 and l.cout <= 512 and l.cin <= 512]
    ws2 = max([0] + [wgrad_ws(i) for i in part._side_wgrad_bf16])
    part.wgrad_ws_b2 = e._storage.view('wgrad_ws_b2', ws2 // 4 + 64)[0] if ws2 else None
    part.wgrad_ws_b3 = e._storage.view('wgrad_ws_b3', ws2 // 4 + 64)[0] if ws2 else None    # second side stream
    if self.Wb is None:
      z = lambda n: torch.zeros(n, dtype=torch.bfloat16, device=e.device)
      self.Wb = [z(l.k_pad * l.n_pad) for l in layers]
      self.WTb = [None] + [z(l.kt_pad * l.nt_pad) for l in layers[1:]]
    # the frequency-domain layers: tables, filter spectra in both operand layouts (kept across shapes), spectra and scratch
    part.fftb = {}
    for i in sorted(part.fftb_layers):
      l = layers[i]
      t_in, t_out, pl, pr = geo[i]
      view = lambda name, numel, dtype=None: e._storage.view('fftb%d_%s' % (i, name), numel, dtype)
      bf = torch.bfloat16
      tables, fresh_tables = view('tables', lib.st_conv1d_fft_table_floats())
      if self._fftb_table_key.get(i) != (l.width, pl):
        fresh_tables = True
      self._fftb_table_key[i] = (l.width, pl)
      ge = lib.st_conv1d_fft_filter_plane_elems(l.width, l.cin_pitch, l.cout)
      g, fresh_g = view('g', ge, bf)
      rows_pad, blocks = ctypes.c_int(), ctypes.c_int()
      call('st_conv1d_fft_plan', l.width, t_out, batch, None, None, ctypes.byref(blocks), None, ctypes.byref(rows_pad))
      f = dict(tables=tables, g=g, gt=view('gt', ge, bf)[0],
               sf=view('sf', lib.st_conv1d_fft_sf_floats(X[i].ref, X[i + 1].ref, l.width), bf)[0],
               zf=view('zf', lib.st_conv1d_fft_zf_floats(dZ[i].ref, l.width), bf)[0],
               dc=view('dc', rows_pad.value * l.n_pad)[0], rows=batch * blocks.value,
               ws=view('ws', lib.st_conv1d_fft_planes_ws(X[i].ref, X[i + 1].ref, l.width, 1) // 4 + 64)[0], pl=pl)
      if fresh_tables:
        call('st_conv1d_fft_tables_f32', l.width, pl, ptr(tables), tables.numel(), e.stream_ptr)
      if fresh_g:
        self._wplanes_fresh = False
      part.fftb[i] = f
    part.table_keys = {i: (layers[i].width, f['pl']) for i, f in part.fftb.items()}       # (the re-entry token, as in SpectralLayers)
    self._fftb_transition(part.fftb, None)
    return part

  def reenter(self, sh):
    self._fftb_transition(sh.mode.fftb, sh.mode.table_keys)

  def refresh_under_ctc(self):
    if not self._wtplanes_fresh and self.WTb is not None:
      self.e._on_side_stream(lambda: self._refresh_bf16_filters(True))

  def refresh_after_update(self):
    if self.Wb is not None:
      self._refresh_wb_after_update()              # the bf16 copies the next forward pass reads

  def prepare_forward_graph(self):
    if not self._wplanes_fresh:
      self._refresh_bf16_filters(False)            # derived operands are rebuilt outside the graph
    self.e._join_side_stream()
    self._wb_ready.clear()                         # (covered by the join above)

  def _use_fft_bf16(self, i, batch, t_out):
    """bf16 activations (configs[3]): the 32-tap 250 -> 2000 layer runs as block DFTs + per-bin products on the bf16 matrix pipe
    (st_conv1d_*_fft_planes, one bf16 plane): 51.5 GFLOP per pass instead of the W-tap kernel's 513.  Only the wide
    long-filter layer: the narrow layers' W-tap bf16 kernels are launch-bound (~30 us), nothing to gain there."""
    e = self.e
    l = e.layers[i]
    return (e.conv_mode == 'bf16' and e.fft_conv and os.environ.get('ST_FFT_BF16', '1') != '0' and i > 0 and
            l.stride == 1 and 16 <= l.width <= 32 and l.n_pad % 128 == 0 and batch * t_out >= e.fft_min_rows)

  def _fftb_transition(self, fftb, table_keys):
    """What entering a shape does that depends on the shape left behind (see SpectralLayers._fft_transition)."""
    for i, key in (table_keys or {}).items():
      if self._fftb_table_key.get(i) != key:
        f = fftb[i]
        call('st_conv1d_fft_tables_f32', key[0], key[1], self.e._ptr(f['tables']), f['tables'].numel(), self.e.stream_ptr)
        self._fftb_table_key[i] = key
    if set(fftb) != self._fftb_prev:
      self._wplanes_fresh = False
      self._wtplanes_fresh = False
    self._fftb_prev = set(fftb)

  def _refresh_bf16_filters(self, transposed, layers=None):
    e, ptr = self.e, self.e._ptr
    fftb = e.shape.mode.fftb
    for i, l in enumerate(e.layers):
      if layers is not None and i not in layers:
        continue
      if i in fftb:
        # a frequency-domain layer: its filter spectra (one bf16 plane, both operand layouts) instead of the two bf16 copies
        if not transposed:
          f = fftb[i]
          call('st_conv1d_fft_filters_planes', ptr(e._slice(e.params, i)[0]), l.width, l.cin, l.cout, l.cin_pitch, ptr(f['tables']),
               ptr(f['g']), ptr(f['gt']), 1, e.stream_ptr)
        continue
      if transposed and i > 0:
        call('st_filters_bwd_bf16', ptr(e._slice(e.params, i)[0]), l.width, l.cin, l.cout, l.cin_pitch, l.cout_pitch,
             ptr(self.WTb[i]), e.stream_ptr)
      elif not transposed:
        call('st_filters_bf16', ptr(e._slice(e.params, i)[0]), l.k_pad, l.n_pad, ptr(self.Wb[i]), e.stream_ptr)
    if layers is not None:
      return
    if transposed:
      self._wtplanes_fresh = True
    else:
      self._wplanes_fresh = True

  def _refresh_wb_after_update(self):
    """After an update: the bottom layer's bf16 filter copy on the compute stream (the next forward pass needs it at
    once), the others on the side stream -- the small copies bottom layer first, the frequency-domain layers' filter spectra
    (L9: a 16 M-weight transform and its second operand layout, 0.16 ms) LAST, an event per layer: the forward pass waits for
    what a layer reads, not for the whole list, and the spectra are built beside the eight layers below them."""
    e = self.e
    L = len(e.layers)
    self._wb_ready = ready = {}
    self._refresh_bf16_filters(False, layers=[0])
    fftb = e.shape.mode.fftb
    order = [i for i in range(1, L) if i not in fftb] + [i for i in range(1, L) if i in fftb]

    def rest():
      for i in order:
        self._refresh_bf16_filters(False, layers=[i])
        ev = torch.cuda.Event()
        ev.record(e.stream)                        # (the side stream `_on_side_stream` has swapped in)
        ready[i] = ev
    e._on_side_stream(rest)
    self._wb_order = order
    self._wplanes_fresh = True

  def forward(self, mask_padding=False):
    """``mask_padding``: the bf16 plane of every layer's output but the last is masked (st_mask_rows on 2-byte elements); no layer
    here hands its successor anything but that plane."""
    e, ptr = self.e, self.e._ptr
    sh, s, main, L = e.shape, e.stream_ptr, e.stream, len(e.layers)
    valid = e._mask_lengths() if mask_padding else None
    X, geo, part, Xb, fftb, Wb = sh.X, sh.geo, sh.mode, sh.mode.Xb, sh.mode.fftb, self.Wb
    ws = part.wgrad_ws_b
    ws_bytes = ws.numel() * 4 if e.split_small_batches else 0
    ready = self._wb_ready
    if not self._wplanes_fresh:
      e._join_side_stream()                          # (a rebuild still running there writes the same buffers)
      ready.clear()
      self._refresh_bf16_filters(False)
    call('st_cast_bf16', ptr(X[0].buf), X[0].buf.numel(), ptr(Xb[0]), s)
    for i, l in enumerate(e.layers):
      last = i + 1 == L
      if i in ready:
        # the side stream works in self._wb_order: the first layers wait for their own copy, the fourth for every small copy
        # (by then they are through; every wait costs the compute stream a few microseconds), a frequency-domain layer for its
        # own spectra
        if i in fftb or i < 3:
          main.wait_event(ready.pop(i))
        else:
          small = [j for j in self._wb_order if j not in fftb]
          main.wait_event(ready[small[-1]])
          for j in small:
            ready.pop(j, None)
      pb = ptr(e._slice(e.params, i)[1])
      if i in fftb and not last:
        f = fftb[i]
        call('st_conv1d_nwc_fwd_fft_planes', X[i].ref, ptr(Xb[i]), ptr(f['gt']), pb, l.width, f['pl'], int(l.relu), X[i + 1].ref,
             ptr(Xb[i + 1]), ptr(f['tables']), ptr(f['sf']), 1, ptr(f['ws']), f['ws'].numel() * 4, s)
      else:
        call('st_conv1d_nwc_fwd_ws_bf16', X[i].ref, ptr(Xb[i]), ptr(Wb[i]), pb, l.width, l.stride, geo[i][2], int(l.relu),
             X[i + 1].ref, None if last else ptr(Xb[i + 1]), ptr(X[i + 1].buf) if last else None, ptr(ws), ws_bytes, s)
      if mask_padding and not last:
        y = X[i + 1]
        plane = _lib.Tensor3(Xb[i + 1].data_ptr(), y.batch, y.frames, y.channels, y.halo, y.t_pitch, y.c_pitch)
        call('st_mask_rows', ctypes.byref(plane), valid(i), 2, s)

  def backward(self, on_layer_done, wanted):
    e, ptr = self.e, self.e._ptr
    e._join_side_stream()
    sh, s, layers, L = e.shape, e.stream_ptr, e.layers, len(e.layers)
    X, dZ, geo, part = sh.X, sh.dZ, sh.geo, sh.mode
    Xb, dZb, fftb, WTb, wgrad_tr = part.Xb, part.dZb, part.fftb, self.WTb, part._wgrad_tr
    ws_b, ws_b2, ws_b3 = part.wgrad_ws_b, part.wgrad_ws_b2, part.wgrad_ws_b3
    if not self._wtplanes_fresh:
      self._refresh_bf16_filters(True)
    call('st_cast_bf16', ptr(dZ[L - 1].buf), dZ[L - 1].buf.numel(), ptr(dZb[L - 1]), s)
    side = False
    for i in reversed(range(L)):
      l = layers[i]
      gf, gb = e._slice(e.grads, i)
      beside = i in part._side_wgrad_bf16         # this layer's filter gradient runs beside its back-prop to the input

      if i in fftb:
        # frequency-domain layer: ONE transform of dz (bf16 spectra + the fp32 block sums) serves the filter gradient, the bias
        # gradient and back-prop to the input
        f = fftb[i]
        call('st_conv1d_fft_dz_spectra_planes', dZ[i].ref, ptr(dZb[i]), l.width, ptr(f['tables']), ptr(f['zf']), 1, ptr(f['dc']), s)
        call('st_conv1d_nwc_bwd_filter_fft_planes', X[i].ref, dZ[i].ref, ptr(f['sf']), ptr(f['zf']), l.width, ptr(f['tables']),
             ptr(gf), 1, ptr(f['ws']), f['ws'].numel() * 4, s)
        call('st_conv1d_fft_bias_grad_dc_f32', ptr(f['dc']), f['rows'], l.cout, l.n_pad, ptr(gb), s)
        if on_layer_done is not None and wanted(i):
          if side:                       # (filter gradients of layers above still on the side streams: same bucket, see below)
            e._join_side_stream()
            side = False
          on_layer_done(i)
        relu_in = layers[i - 1].relu
        call('st_conv1d_nwc_bwd_data_fft_planes', dZ[i].ref, ptr(f['zf']), ptr(f['g']), l.width, f['pl'], X[i].ref if relu_in else None,
             ptr(Xb[i]) if relu_in else None, dZ[i - 1].ref, ptr(dZb[i - 1]), ptr(f['tables']), 1, ptr(f['ws']), f['ws'].numel() * 4, s)
        continue

      # (run now or on a side stream: `e.stream_ptr` is read when it runs)
      def filter_gradient(i=i, l=l, gf=gf, gb=gb, ws=(ws_b3 if (i % 2 == 1 and ws_b3 is not None) else ws_b2) if beside else ws_b):
        call('st_conv1d_nwc_bwd_filter_tr_bf16' if wgrad_tr[i] else 'st_conv1d_nwc_bwd_filter_bf16', X[i].ref, ptr(Xb[i]),
             dZ[i].ref, ptr(dZb[i]), l.width, l.stride, geo[i][2], ptr(gf), ptr(gb), ptr(ws), ws.numel() * 4, e.stream_ptr)
      if beside:
        # two side streams take the chains in turn (each needs only its own layer's tensors): with all seven on one
        # stream that stream, not back-prop to the input, set the length of the backward pass of the narrow layers
        e._on_side_stream(filter_gradient, second=(i % 2 == 1 and ws_b3 is not None))
        side = True
      else:
        filter_gradient()
        if on_layer_done is not None and wanted(i):
          if side:
            # the bucket this layer completes also holds layers whose filter gradients are still in flight on the side
            # streams (bottom bucket L0..L3: L1-L3 run beside back-prop, L0 does not); the exchange is ordered behind the
            # compute stream only
            e._join_side_stream()
            side = False
          on_layer_done(i)
      if i > 0:
        relu_in = layers[i - 1].relu
        call('st_conv1d_nwc_bwd_data_bf16', dZ[i].ref, ptr(dZb[i]), ptr(WTb[i]), l.width, geo[i][2], X[i].ref if relu_in else None,
             ptr(Xb[i]) if relu_in else None, dZ[i - 1].ref, ptr(dZb[i - 1]), ptr(ws_b), ws_b.numel() * 4, s)
      if beside and on_layer_done is not None and wanted(i):
        e._join_side_stream()
        side = False
        on_layer_done(i)
    if side:
      e._join_side_stream()
