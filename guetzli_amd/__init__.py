"""guetzli_amd -- MI355X (gfx950) implementation of Guetzli's block-parallel hot path
(block DCT / quantise / IDCT round trip + butteraugli distance map) behind the C ABI of
include/guetzli_amd.h.  See DESIGN.md."""
from .capi import Context, GuetzliAmdError, Library, load  # noqa: F401
from .encoder import Comparator, HostLibrary, adaptive_quantization, blend_on_background, butteraugli, butteraugli_batch, butteraugli_linear, decode, decode_batch, decode_batch_info, decode_info, fuzzy_class, fuzzy_inverse, heatmap, load_host, mask, opsin_dynamics, process, process_jpeg, process_many, process_png, read_png  # noqa: F401

__all__ = ["Context", "GuetzliAmdError", "Library", "load", "HostLibrary", "load_host", "decode", "decode_batch", "decode_batch_info", "decode_info", "butteraugli", "butteraugli_batch", "butteraugli_linear", "Comparator", "heatmap", "fuzzy_class", "fuzzy_inverse", "opsin_dynamics", "mask", "adaptive_quantization", "process", "process_many", "process_png", "process_jpeg", "read_png"]
