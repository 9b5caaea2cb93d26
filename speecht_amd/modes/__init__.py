"""Arithmetic modes of the Wav2Letter engine: what each one allocates beyond the shared buffers, and its launch sequences.

  fp32     exact-fp32 MFMA kernels; nine of the eleven layers in the frequency domain (BASELINE configs[1], the headline)
  bf16x6   the same with the wide 1 x 1 layers as fp32-accurate three-piece bf16 products (experimental, opt-in)
  bf16     bf16 activations and activation gradients, fp32 masters / accumulation / CTC / Adam (BASELINE configs[3])

A mode object owns the state of its arithmetic that outlives a shape (derived weight copies such as `Wb`, freshness flags, events,
transform-table keys: all created in its `__init__`); what it needs per (batch, frames) is the object its `alloc` returns, kept by
the engine in `ShapeState.mode` (`fft`, `Xb`, `wgrad_ws`, ...).  Outside readers still find `eng.fft`, `eng.Xb`, `eng.Wb` through the
engine's read-only `__getattr__`; code in the package names `engine.shape.mode.fft` / `engine.mode.Wb`.
"""
from .bf16 import Bf16Mode
from .bf16x6 import Bf16x6Mode
from .fp32 import Fp32Mode

MODES = {'fp32': Fp32Mode, 'bf16x6': Bf16x6Mode, 'bf16': Bf16Mode}


def make_mode(engine):
  return MODES[engine.conv_mode](engine)
