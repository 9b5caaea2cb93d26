"""Frequency-domain layers (csrc/conv_fft.hip) of the fp32 and bf16x6 modes: which layers take the path for a shape, their
tables / filter spectra / scratch, and the refresh of the filter spectra after an update."""
import ctypes

import torch

from .. import _lib
from .._lib import Tensor3, call


class SpectralLayers:
  """Mixin of `Fp32Mode`: `fft[i]` (in the mode's part of the ShapeState) describes layer i on the frequency path (tables, the ONE
  set of filter spectra `gfwd`, input / gradient spectra, scratch per stream).  Across shapes the mode keeps `_gfwd_fresh` /
  `_gfwd_ready` (the spectra follow the weights; events of a rebuild on the side stream), `_fft_table_key` (whose tables lie in
  each layer's buffer) and `_fft_prev` (the set of layers of the shape left behind); `Fp32Mode.__init__` creates them."""

  def _polyphase(self, i, geo):
    """A stride-2 layer as a stride-1 layer on the polyphase view of its input: x read as [B][T/2][2 * c_pitch] (frame
    pairs as channels), y[t] = sum_w F[w] x[2t + w - pl] = sum_{j,p} F[2j + p - shift] X2[t + j - pl2][p] with
    pl2 = ceil(pl / 2), shift = 2 pl2 - pl: width2 = ceil((W + shift) / 2) taps whose packed filters are the layer's
    own rows moved down by `shift` channel blocks (zeros around them).  Returns (width2, pl2, shift) or None."""
    l = self.e.layers[i]
    if l.stride != 2:
      return None
    pl = geo[i][2]
    pl2 = (pl + 1) // 2
    shift = 2 * pl2 - pl
    return (l.width + shift + 1) // 2, pl2, shift

  def _use_fft(self, i, batch, geo):
    e = self.e
    l = e.layers[i]
    wide = l.stride == 1 and l.width >= 16
    if not (e.fft_conv and e.conv_mode in ('fp32', 'bf16x6') and l.n_pad % 128 == 0 and
            batch * geo[i][1] >= (e.fft_min_rows if wide else e.fft_min_rows_narrow)):
      return False
    if l.stride == 2:        # first layer of the model (48 taps, stride 2): 25 polyphase taps over 2 x 80 channels
      width2 = self._polyphase(i, geo)[0]
      return i == 0 and e.fft_first_layer and e.fft_min_width <= width2 <= 32
    return i > 0 and l.stride == 1 and e.fft_min_width <= l.width <= 32 and l.nt_pad % 128 == 0

  def _alloc_fft(self, sh, part):
    """Per frequency-domain layer: the transform tables and the filter spectra in both operand layouts (functions of
    the layer only: kept across shapes), the input / gradient spectra and one scratch area (sized by the shape)."""
    lib = _lib.load()
    e, ptr, X, dZ, batch = self.e, self.e._ptr, sh.X, sh.dZ, sh.batch
    part.fft = {}
    for i, l in enumerate(e.layers):
      t_in, t_out, pl, pr = sh.geo[i]
      if i not in part.fft_layers:
        continue
      view = lambda name, numel: e._storage.view('fft%d_%s' % (i, name), numel)
      f = dict(x=X[i].desc, width=l.width, pl=pl, cin=l.cin, cin_pitch=l.cin_pitch, shift=None)
      if l.stride == 2:
        width2, pl2, shift = self._polyphase(i, sh.geo)
        x = X[i]
        assert x.halo % 2 == 0 and x.t_pitch % 2 == 0
        cp2 = 2 * x.c_pitch
        f.update(x=Tensor3(x.buf.data_ptr(), batch, t_out, cp2, x.halo // 2, x.t_pitch // 2, cp2), width=width2, pl=pl2,
                 cin=cp2, cin_pitch=cp2, shift=shift)
        # the layer's packed filters between zero blocks, and the gradient in the same layout
        rows = 2 * width2 * x.c_pitch * l.n_pad
        f['packed2'], fresh_p = view('packed2', rows)
        f['dpacked2'] = view('dpacked2', rows)[0]
        if fresh_p:
          f['packed2'].zero_()
          self._gfwd_fresh = False
      f['xref'] = ctypes.byref(f['x'])
      tables, fresh_tables = view('tables', lib.st_conv1d_fft_table_floats())
      # the tables are functions of (taps, left padding): a new shape or another model may change either for the same
      # layer index, so the pair is kept with them
      if self._fft_table_key.get(i) != (f['width'], f['pl']):
        fresh_tables = True
      self._fft_table_key[i] = (f['width'], f['pl'])
      # ONE set of filter spectra: back-prop to the input reads it as a transposed operand (csrc/conv_fft.hip)
      gfwd, fresh_f = view('gfwd', lib.st_conv1d_fft_filter_floats(f['width'], f['cin_pitch'], l.cout))
      f.update(tables=tables, gfwd=gfwd, sf=view('sf', lib.st_conv1d_fft_sf_floats(f['xref'], X[i + 1].ref, f['width']))[0],
               zf=view('zf', lib.st_conv1d_fft_zf_floats(dZ[i].ref, f['width']))[0],
               ws=view('ws', lib.st_conv1d_fft_ws(f['xref'], X[i + 1].ref, f['width']) // 4 + 64)[0])
      # (the wide 32-tap layer stays on one stream: its chain side by side, or only its HBM-bound inverse transform of the
      # lag products beside back-prop's products, both measured slower: 7.37 -> 7.43 ms)
      if e.side_filter_gradient and i > 0 and l.cout <= 512:
        f['ws2'] = view('ws2', lib.st_conv1d_fft_ws(f['xref'], X[i + 1].ref, f['width']) // 4 + 64)[0]
      if fresh_tables:
        call('st_conv1d_fft_tables_f32', f['width'], f['pl'], ptr(tables), tables.numel(), e.stream_ptr)
      if fresh_f:
        self._gfwd_fresh = False
      part.fft[i] = f
    # (the re-entry token: what `_fft_transition` checks the tables in the buffers against when this shape comes round again)
    part.table_keys = {i: (f['width'], f['pl']) for i, f in part.fft.items()}
    self._fft_transition(part.fft, None)

  def _fft_transition(self, fft, table_keys):
    """What entering a shape (its layers: ``fft``) does that depends on the shape left behind.  ``table_keys``: {layer: (taps,
    left padding)} of a cached description being put back -- its tables are rebuilt if another shape has left different ones in
    the layer's buffer (a fresh description has just done that itself)."""
    for i, key in (table_keys or {}).items():
      if self._fft_table_key.get(i) != key:
        f = fft[i]
        call('st_conv1d_fft_tables_f32', f['width'], f['pl'], self.e._ptr(f['tables']), f['tables'].numel(), self.e.stream_ptr)
        self._fft_table_key[i] = key
    if set(fft) != self._fft_prev:                               # a layer (re)joined the path: its spectra may be stale
      self._gfwd_fresh = False
      self._packed_t_fresh = False                               # (and a layer that left it needs its flipped copy again)
    self._fft_prev = set(fft)

  def _refresh_fft_filters(self, layers=None):
    """Filter spectra of the frequency-domain layers (all, or the given ones) from the current weights, in layer
    order; on a side stream an event is recorded after each layer so that the forward pass waits for the layer it is
    about to run, not for all.  (Back-prop to the input reads the same spectra, transposed.)"""
    e, ptr = self.e, self.e._ptr
    sh, stream = e.shape, e.stream
    if layers is None:
      self._gfwd_ready = {}
    for i, f in sh.mode.fft.items():
      if layers is not None and i not in layers:
        continue
      l = e.layers[i]
      pf = e._slice(e.params, i)[0]
      if f['shift'] is not None:
        cp = sh.X[i].c_pitch
        n = l.width * cp * l.n_pad
        with torch.cuda.stream(stream):
          f['packed2'][f['shift'] * cp * l.n_pad:f['shift'] * cp * l.n_pad + n].copy_(pf[:n], non_blocking=True)
        pf = f['packed2']
      call('st_conv1d_fft_filters_f32', ptr(pf), f['width'], f['cin'], l.cout, f['cin_pitch'], ptr(f['tables']), ptr(f['gfwd']),
           e.stream_ptr)
      if stream is e._side:
        ev = torch.cuda.Event()
        ev.record(stream)
        self._gfwd_ready[i] = ev
    self._gfwd_fresh = True

  def refresh_after_update(self):
    """The forward filter spectra for the next pass: the bottom layer's spectra on the compute stream (the next step needs them at once; a
    cross-stream wait there costs more than the 25 us of work), the others on the side stream, bottom layer first."""
    sh = self.e.shape
    if sh is not None and sh.mode.fft:
      fft = sh.mode.fft
      first = min(fft)
      self._gfwd_ready = {}
      self._refresh_fft_filters(layers=[first])
      rest = [i for i in fft if i != first]
      if rest:
        self.e._on_side_stream(lambda: self._refresh_fft_filters(layers=rest))

  def _wait_gfwd(self, i=None):
    """The compute stream waits for the forward filter spectra of layer i (None: of every layer) if they were rebuilt on
    the side stream after the update.  The side stream works bottom layer first: the first three frequency-domain layers
    wait for their own spectra, the fourth for all that remain (by then the side stream is through, and every wait
    costs the compute stream a few microseconds)."""
    ready = self._gfwd_ready
    if not ready:
      return
    order = sorted(self.e.shape.mode.fft)
    if i is not None and i in order and order.index(i) >= 3:
      i = None
    keys = [k for k in ready if i is None or k <= i]
    if keys:
      self.e.stream.wait_event(ready[max(keys)])
      for k in keys:
        del ready[k]
