"""Shared by tests/test_device_alpha_emu.py (CPU emulation: "device memory" is host memory) and
tests/test_device_alpha_gpu.py (torch tensors on the MI355X): device-resident pixels with alpha and 16-bit samples
(gz_device_pixels) -- the rule restated in numpy, the layouts an alpha pointer can describe, and the raw samples of the
three PNG fixtures of tests/golden/degenerate/, rebuilt as tools/gen_goldens.py:png_fixtures builds them.

The rule: the byte of a sample is the value (uint8), v >> 8 (uint16: the high byte, libpng's STRIP_16), or
device_input_cases.expected_bytes (the three float types); with alpha byte a, colour byte v and background byte bg
    out = (v * a + bg * (255 - a) + 128) // 255        an integer division of non-negative numbers
which is the reference's BlendOnBlack (guetzli.cc:42-44) at bg = 0.  Storage is kept as in device_input_cases: uint8,
float32, or uint16 -- the integers of "uint16", the bit patterns of float16 / bfloat16."""
import hashlib
import json
import os

import numpy as np

import device_input_cases as dic
import images

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = ("uint8", "uint16", "float32", "float16", "bfloat16")
STORAGE = dict(dic.STORAGE, uint16=np.uint16)
KINDS = ("HWC_rgba", "CHW_rgba", "GA_interleaved", "CHW_ga", "alpha_apart")
LAYOUTS = tuple(k + s for k in KINDS for s in ("", "_crop", "_base1"))
WIDTHS = (1, 3, 4, 5, 15, 16, 17, 33, 61, 64, 67)
HEIGHTS = (1, 2, 9)


def sample_bytes(storage, dtype):
    """The byte of every sample."""
    if dtype == "uint16":
        return (storage >> np.uint16(8)).astype(np.uint8)
    return dic.expected_bytes(storage, dtype)


def blend(v, a, bg):
    """(v * a + bg * (255 - a) + 128) // 255 on bytes; bg: one byte or three (the last axis of v)."""
    v, a, bg = np.asarray(v, np.uint32), np.asarray(a, np.uint32), np.asarray(bg, np.uint32)
    return ((v * a + bg * (np.uint32(255) - a) + np.uint32(128)) // np.uint32(255)).astype(np.uint8)


def expected_rgb(colour, alpha, dtype, bg=(0, 0, 0)):
    """uint8 [h][w][3] of colour storage [h][w][3] (grey: [h][w][1]) and alpha storage [h][w], or alpha = None."""
    v = sample_bytes(colour, dtype)
    if v.shape[2] == 1:
        v = np.repeat(v, 3, axis=2)
    if alpha is None:
        return v
    return blend(v, sample_bytes(alpha, dtype)[..., None], bg)


def random_storage(dtype, n, rng):
    if dtype == "uint16":
        return rng.integers(0, 1 << 16, n, dtype=np.uint16)
    return dic.random_storage(dtype, n, rng)


def random_alpha(dtype, n, rng):
    """Alpha samples: as the colours', with the two ends (transparent, opaque) a third of the time."""
    a = random_storage(dtype, n, rng)
    ends = {"uint8": (0, 255), "uint16": (0, 0xFFFF), "float32": (0.0, 1.0), "float16": (0, 0x3C00), "bfloat16": (0, 0x3F80)}[dtype]
    pick = rng.integers(0, 6, n)
    a = np.where(pick == 0, np.array(ends[0], a.dtype), a)
    return np.where(pick == 1, np.array(ends[1], a.dtype), a).astype(a.dtype)


class Source:
    """storage / offset / strides: the colours, as device_input_cases.Source; alpha_storage / alpha_offset: the buffer
    that holds the alpha samples (the colours' own, or another) and the element of it that is pixel (0, 0)'s.
    colour: storage [h][w][3] or [h][w][1] (grey); alpha: storage [h][w]."""

    def __init__(self, storage, offset, strides, alpha_storage, alpha_offset, w, h, dtype, colour, alpha):
        self.storage, self.offset, self.strides = storage, offset, strides
        self.alpha_storage, self.alpha_offset = alpha_storage, alpha_offset
        self.w, self.h, self.dtype, self.colour, self.alpha = w, h, dtype, colour, alpha
        self.itemsize = storage.dtype.itemsize

    def expected(self, bg=(0, 0, 0)):
        return expected_rgb(self.colour, self.alpha, self.dtype, bg)


def lay_out(colour, alpha, dtype, layout):
    """The pixels placed in fresh, poisoned buffers (64-byte aligned, as a device allocation is):
      HWC_rgba        [h][w][4], alpha = data + 3             CHW_rgba  [4][h][w], alpha = the fourth plane
      GA_interleaved  [h][w][2], stride_c = 0, alpha = data + 1   CHW_ga    [2][h][w], stride_c = 0
      alpha_apart     colours [3][h][w], the alpha samples [h][w] in a buffer of their own
    *_crop: a view into a canvas two rows higher whose rows are a multiple of 16 pixels (the 16-byte paths stay open);
    *_base1: everything one element further on (element by element).  Grey kinds use channel 0 of `colour`."""
    h, w = alpha.shape
    st = STORAGE[dtype]
    poison = 0xAB if st != np.float32 else np.float32(np.nan)
    base1 = 1 if layout.endswith("_base1") else 0
    crop = layout.endswith("_crop")
    kind = layout[:-6] if base1 else layout[:-5] if crop else layout
    H, W, y0, x0 = (h + 2, (w + 16 + 15) // 16 * 16, 1, 16) if crop else (h, w, 0, 0)
    first = y0 * W + x0
    rows, cols = slice(y0, y0 + h), slice(x0, x0 + w)
    grey = kind in ("GA_interleaved", "CHW_ga")
    logical = np.ascontiguousarray(colour[:, :, :1]) if grey else colour
    nch = {"HWC_rgba": 4, "CHW_rgba": 4, "GA_interleaved": 2, "CHW_ga": 2, "alpha_apart": 3}[kind]
    buf = dic.aligned_empty(H * W * nch + base1, st, poison)
    abuf = buf
    if kind in ("HWC_rgba", "GA_interleaved"):
        canvas = buf[base1:].reshape(H, W, nch)
        canvas[rows, cols, :nch - 1] = logical
        canvas[rows, cols, nch - 1] = alpha
        offset = base1 + first * nch
        strides, aoff = (nch * W, nch, 0 if grey else 1), offset + nch - 1
    else:
        canvas = buf[base1:].reshape(nch, H, W)
        canvas[:logical.shape[2], rows, cols] = logical.transpose(2, 0, 1)
        offset = base1 + first
        strides = (W, 1, 0 if grey else H * W)
        if kind == "alpha_apart":
            abuf = dic.aligned_empty(H * W + base1, st, poison)
            abuf[base1:].reshape(H, W)[rows, cols] = alpha
            aoff = base1 + first
        else:
            canvas[nch - 1, rows, cols] = alpha
            aoff = offset + (nch - 1) * H * W
    return Source(buf, offset, strides, abuf, aoff, w, h, dtype, logical, alpha)


def lay_out_opaque(colour, dtype, layout):
    """An opaque image as device_input_cases lays it out (its layouts); that module does not know "uint16", whose
    storage is float16's."""
    src = dic.lay_out(colour, "float16" if dtype == "uint16" else dtype, layout)
    src.dtype = dtype
    return src


def parity_sources(dtype, layout, seed=11):
    """The sources of one (dtype, layout) pack-parity test, each with a random background."""
    rng = np.random.default_rng(seed)
    for h in HEIGHTS:
        for w in WIDTHS:
            colour = random_storage(dtype, h * w * 3, rng).reshape(h, w, 3)
            alpha = random_alpha(dtype, h * w, rng).reshape(h, w)
            yield lay_out(colour, alpha, dtype, layout), tuple(int(v) for v in rng.integers(0, 256, 3))


EXHAUSTIVE_BACKGROUNDS = ((0, 0, 0), (1, 1, 1), (127, 127, 127), (128, 128, 128), (254, 254, 254), (255, 255, 255), (3, 200, 77))


def every_v_a_pair():
    """uint8 colour [256][256][3] and alpha [256][256]: pixel (a, v) has the value v in every channel and the alpha a."""
    a, v = np.mgrid[0:256, 0:256]
    return np.ascontiguousarray(np.repeat(v[..., None], 3, axis=2).astype(np.uint8)), a.astype(np.uint8)


def every_u16_pattern():
    """uint16 colour [256][256][3] and alpha [256][256]: every pattern as a value (each channel in another order) and as
    an alpha."""
    b = np.arange(1 << 16, dtype=np.uint16)
    return dic.all_16bit_patterns(), np.ascontiguousarray(np.roll(b, 4321).reshape(256, 256))


# ------------------------------------------------------------------ the PNG fixtures ----
def fixture(name):
    with open(os.path.join(HERE, "golden", "degenerate", name + ".json")) as f:
        return json.load(f)


def fixture_samples():
    """{fixture name: (samples [120][160][channels], dtype)}: what tools/gen_goldens.py:png_fixtures hands its PNG writer
    -- the raw samples a decoder would put on the GPU.  The rule turns each into the fixture's rgb_sha256, the pixels the
    unmodified reference's ReadPNG made of the file: that pins this module to the reference without running it."""
    b = images.bees()
    h, w = 120, 160
    rgb = b[60:60 + h, 140:140 + w].astype(np.uint32)
    yy, xx = np.mgrid[0:h, 0:w]
    alpha = ((xx * 255) // (w - 1) + (yy * 255) // (h - 1)) // 2
    rgba = np.concatenate([rgb, alpha[..., None].astype(np.uint32)], -1)
    low = images.noise(w, h, seed=7).astype(np.uint32)
    rgb16 = rgb * 256 + low
    ga16 = np.stack([rgb[..., 1] * 257, (65535 - alpha * 257)], -1).astype(np.uint32)
    out = {"png_rgba8_160x120_q95": (np.ascontiguousarray(rgba.astype(np.uint8)), "uint8"),
           "png_rgb16_160x120_q95": (np.ascontiguousarray(rgb16.astype(np.uint16)), "uint16"),
           "png_greyalpha16_interlaced_160x120_q90": (np.ascontiguousarray(ga16.astype(np.uint16)), "uint16")}
    for name, (s, dtype) in out.items():
        exp = fixture_rgb(s, dtype)
        assert hashlib.sha256(exp.tobytes()).hexdigest() == fixture(name)["rgb_sha256"], name
    return out


def fixture_rgb(samples, dtype):
    """The rule on samples [h][w][2 | 3 | 4] over black."""
    ch = samples.shape[2]
    if ch == 3:
        return expected_rgb(samples, None, dtype)
    return expected_rgb(samples[:, :, :ch - 1], samples[:, :, ch - 1], dtype)
