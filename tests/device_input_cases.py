"""Shared by tests/test_device_input_emu.py (CPU emulation: "device memory" is host memory) and
tests/test_device_input_gpu.py (torch tensors on the MI355X): the ingest rule restated in numpy, the element contents,
and the layouts a gz_device_image can describe.

A source is kept as STORAGE: uint8, float32, or the uint16 bit patterns of float16 / bfloat16, so that the same numpy
buffers serve both suites (numpy has no bfloat16) and every bit pattern can be written down."""
import numpy as np

DTYPES = ("uint8", "float32", "float16", "bfloat16")
STORAGE = {"uint8": np.uint8, "float32": np.float32, "float16": np.uint16, "bfloat16": np.uint16}
LAYOUTS = ("HWC", "CHW", "HWC_crop", "CHW_crop", "grey", "HWC_base1", "CHW_crop_base1")
WIDTHS = (1, 3, 4, 5, 33, 61, 64, 67)
HEIGHTS = (1, 2, 9)


def widen(storage, dtype):
    """The elements as float32, exactly (uint8: the integers themselves)."""
    if dtype == "uint8":
        return storage
    if dtype == "float32":
        return storage.astype(np.float32, copy=False)
    if dtype == "float16":
        return storage.view(np.float16).astype(np.float32)
    return (storage.astype(np.uint32) << np.uint32(16)).view(np.float32)


def expected_bytes(storage, dtype):
    """The issue's rule: np.rint(np.clip(np.where(np.isnan(v), 0, v), 0, 255)) with v = x.astype(f32) * f32(255)."""
    if dtype == "uint8":
        return storage.astype(np.uint8)
    with np.errstate(all="ignore"):
        v = widen(storage, dtype) * np.float32(255)
        assert v.dtype == np.float32
        return np.rint(np.clip(np.where(np.isnan(v), np.float32(0), v), 0, 255)).astype(np.uint8)


def from_bytes(rgb, dtype):
    """Storage whose elements are k / 255 for the bytes k of `rgb`: the rule maps them back to k."""
    if dtype == "uint8":
        return np.ascontiguousarray(rgb, np.uint8)
    x = rgb.astype(np.float32) / np.float32(255)
    if dtype == "float32":
        return x
    if dtype == "float16":
        return x.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32)   # bfloat16: round to nearest even on the upper 16 bits
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def f32_specials():
    """+-0, denormals, NaN, +-inf, +-1e30, 1, nextafter(1, 2); around every tie (k + 0.5) / 255 the five nearest
    floats -- both sides of each tie, and the tie itself where x * 255 lands on it; random bit patterns."""
    one = np.float32(1)
    vals = [0.0, -0.0, 1e-45, -1e-45, 1e-39, np.nan, -np.nan, np.inf, -np.inf, -1e30, 1e30, 1.0, np.nextafter(one, np.float32(2)),
            np.nextafter(one, np.float32(0)), 0.5, -1.0, 2.0, 1.0 / 255, 254.5 / 255, 255.5 / 255]
    out = [np.array(vals, np.float32)]
    k = (np.arange(255, dtype=np.float64) + 0.5) / 255.0
    c = k.astype(np.float32)
    lo1 = np.nextafter(c, np.float32(0)); lo2 = np.nextafter(lo1, np.float32(0))
    hi1 = np.nextafter(c, np.float32(2)); hi2 = np.nextafter(hi1, np.float32(2))
    out += [lo2, lo1, c, hi1, hi2]
    rng = np.random.default_rng(20261019)
    out.append(rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32).view(np.float32))
    return np.concatenate(out)


def random_storage(dtype, n, rng):
    """n elements: bytes; for the floats a mix of [0, 1] values, the specials above and arbitrary bit patterns."""
    if dtype == "uint8":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if dtype == "float32":
        sp = f32_specials()
        pick = rng.integers(0, 3, n)
        uni = rng.random(n, dtype=np.float32)
        return np.where(pick == 0, uni, sp[rng.integers(0, sp.size, n)]).astype(np.float32)
    bits = rng.integers(0, 1 << 16, n, dtype=np.uint16)
    unit = from_bytes(rng.integers(0, 256, n, dtype=np.uint8), dtype)
    return np.where(rng.integers(0, 2, n) == 0, bits, unit).astype(np.uint16)


def all_16bit_patterns():
    """uint16 [256][256][3]: every pattern in every channel, each channel in another order."""
    b = np.arange(1 << 16, dtype=np.uint16)
    return np.ascontiguousarray(np.stack([b, b[::-1], np.roll(b, 12345)], -1).reshape(256, 256, 3))


def aligned_empty(n, dtype, fill):
    """n elements whose first is 64-byte aligned (what a device allocation gives), filled with `fill`."""
    item = np.dtype(dtype).itemsize
    raw = np.empty(n * item + 64, np.uint8)
    off = (-raw.ctypes.data) % 64
    a = raw[off:off + n * item].view(dtype)
    a[...] = fill
    return a


class Source:
    """storage: the flat buffer; offset: the element of the buffer that is (0, 0, 0); strides: (y, x, c) in elements."""

    def __init__(self, storage, offset, strides, w, h, dtype, logical):
        self.storage, self.offset, self.strides = storage, offset, strides
        self.w, self.h, self.dtype = w, h, dtype
        self.logical = logical              # storage [h][w][3] of the image itself
        self.itemsize = storage.dtype.itemsize


def lay_out(logical, dtype, layout):
    """The image `logical` (storage [h][w][3]; for "grey" its channel 0 counts) placed in a fresh buffer in `layout`:
    HWC / CHW contiguous; *_crop: a view into a larger canvas whose rows are a multiple of 16 pixels (the pitch keeps the
    16-byte path open while the row is longer than the image); grey: [h][w] with stride_c = 0; *_base1: the same one
    element further on, so that the base address is not 16-byte aligned."""
    h, w, _ = logical.shape
    st = STORAGE[dtype]
    poison = 0xAB if st != np.float32 else np.float32(np.nan)
    base1 = 1 if layout.endswith("_base1") else 0
    kind = layout[:-6] if base1 else layout
    cw, ch = (w + 16 + 15) // 16 * 16, h + 2
    if kind == "HWC":
        buf = aligned_empty(h * w * 3 + base1, st, poison)
        buf[base1:] = logical.ravel()
        return Source(buf, base1, (3 * w, 3, 1), w, h, dtype, logical)
    if kind == "CHW":
        buf = aligned_empty(h * w * 3 + base1, st, poison)
        buf[base1:] = logical.transpose(2, 0, 1).ravel()
        return Source(buf, base1, (w, 1, h * w), w, h, dtype, logical)
    if kind == "HWC_crop":
        buf = aligned_empty(ch * cw * 3 + base1, st, poison)
        canvas = buf[base1:].reshape(ch, cw, 3)
        canvas[1:1 + h, 16:16 + w] = logical
        return Source(buf, base1 + (cw + 16) * 3, (3 * cw, 3, 1), w, h, dtype, logical)
    if kind == "CHW_crop":
        buf = aligned_empty(3 * ch * cw + base1, st, poison)
        canvas = buf[base1:].reshape(3, ch, cw)
        canvas[:, 1:1 + h, 16:16 + w] = logical.transpose(2, 0, 1)
        return Source(buf, base1 + cw + 16, (cw, 1, ch * cw), w, h, dtype, logical)
    assert kind == "grey"
    grey = np.repeat(logical[:, :, :1], 3, axis=2)
    buf = aligned_empty(h * w, st, poison)
    buf[...] = grey[:, :, 0].ravel()
    return Source(buf, 0, (w, 1, 0), w, h, dtype, grey)


def parity_sources(dtype, layout, seed=7):
    """The sources of one (dtype, layout) pack-parity test: every width x height of the issue, random content."""
    rng = np.random.default_rng(seed)
    for h in HEIGHTS:
        for w in WIDTHS:
            logical = random_storage(dtype, h * w * 3, rng).reshape(h, w, 3)
            yield lay_out(logical, dtype, layout)


def exhaustive_sources(dtype):
    """Float content that leaves nothing out: every 16-bit pattern (float16, bfloat16) as a 256 x 256 image, the
    float32 specials as a 64-wide one; contiguous HWC and CHW (the 16-byte paths) and an unaligned base (element-wise)."""
    if dtype == "float32":
        sp = f32_specials()
        n = -(-sp.size // (64 * 3)) * 64 * 3
        logical = np.resize(sp, n).reshape(-1, 64, 3)
    else:
        logical = all_16bit_patterns()
    for layout in ("HWC", "CHW", "HWC_base1"):
        yield lay_out(logical, dtype, layout)
