"""What the engine core asks of an arithmetic mode."""


class ModeBase:
  """A mode = the operands derived from the weights and the activations that only this arithmetic needs, plus the launch
  sequences of the forward and the backward pass.  Its state has two homes: what outlives a shape (derived weight copies, their
  freshness flags and events, which transform tables lie in the buffers) is an attribute of the mode object, created in its
  `__init__`; what is a function of the shape is the object `alloc` returns, which the engine keeps in `ShapeState.mode` and never
  looks into.  The shared buffers, streams and events are the engine's (`self.e`)."""
  cache_shapes = True             # False: `alloc` decides things that are not functions of the shape -- described anew every time
  fft = fftb = {}                 # (what `engine.fft` / `engine.fftb` show an outside reader where the mode has no such layers)

  def __init__(self, engine):
    self.e = engine

  # ---- the interface -------------------------------------------------------------------------------------------
  def alloc(self, sh):
    """This mode's part of the ShapeState under construction (X, dZ, geo exist; `sh` is not the engine's current shape yet).
    Byte ranges another shape may overwrite are logged in `sh.ranges`."""
    raise NotImplementedError

  def reenter(self, sh):
    """A cached shape is current again: redo what `alloc` does that depends on the shape LEFT BEHIND (freshness flags)."""

  def weights_changed(self):
    """The weights were written (an update, `set_weights`): everything derived from them is stale."""
    raise NotImplementedError

  def forget_tables(self):
    """A tuning knob was flipped: the transform tables in the layers' buffers are rebuilt by the next description."""

  masks_padding = False           # True: `forward(mask_padding=True)` is implemented (the engine raises for a mode without it)

  def forward(self, mask_padding=False):
    """``mask_padding``: zero every utterance's rows past its own length after every layer but the last
    (`Wav2LetterEngine.forward`); the next layer must then read those time-domain rows, not operands handed over beside them.
    Without the flag the launch sequence is exactly the unmasked one."""
    raise NotImplementedError

  def backward(self, on_layer_done, wanted):
    raise NotImplementedError

  def refresh_under_ctc(self):
    """Operands of back-prop derived from the weights, rebuilt on the side stream while the CTC recursion runs."""

  def refresh_after_update(self):
    """Operands of the NEXT forward pass derived from the weights, right after clip + Adam."""

  def prepare_forward_graph(self):
    """Everything `forward()` would rebuild or wait for on demand, done before a forward graph is captured / replayed."""
