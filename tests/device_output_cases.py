"""Shared by tests/test_device_output_emu.py (CPU emulation: "device memory" is host memory) and
tests/test_device_output_gpu.py (memory of the MI355X): the emit rule of gz_device_output restated in numpy, the
destinations a gz_device_output can describe -- each inside a buffer pre-filled with a sentinel pattern, so that a write
outside the image's (y, x, c) set shows -- coefficients to decode, and a reader of the reference's JPEG dump.

Elements are kept as STORAGE, as tests/device_input_cases.py keeps them: uint8, float32, uint16 for uint16 itself and
for the bit patterns of float16 / bfloat16 (numpy has no bfloat16)."""
import struct

import numpy as np

import device_input_cases as dic

DTYPES = ("uint8", "uint16", "float32", "float16", "bfloat16")
STORAGE = dict(dic.STORAGE, uint16=np.uint16)
# HWC / CHW contiguous; *_crop: a view inside a larger canvas whose pitch keeps the 16-byte stores open; *_base1: one
# element further on, so that the base address is not 16-byte aligned and every store is element-wise; HWC_pitch1: a row
# pitch that is no multiple of the vector (rows start unaligned); WHC: x outermost, an order no fast path knows
LAYOUTS = ("HWC", "CHW", "HWC_crop", "CHW_crop", "HWC_base1", "CHW_crop_base1", "HWC_pitch1", "WHC")
WIDTHS = (1, 3, 4, 5, 15, 16, 17, 33, 61, 64, 67)
HEIGHTS = (1, 2, 9)


def emitted(rgb, dtype):
    """The issue's value rule: the storage elements of the bytes `rgb`."""
    b = np.asarray(rgb, np.uint8)
    if dtype == "uint8":
        return b.copy()
    if dtype == "uint16":
        return b.astype(np.uint16) * np.uint16(257)
    f = b.astype(np.float32) / np.float32(255)          # the IEEE division, NOT b * (1 / 255.f)
    assert f.dtype == np.float32
    if dtype == "float32":
        return f
    if dtype == "float16":
        return f.astype(np.float16).view(np.uint16)     # numpy rounds to nearest, ties to even
    u = f.view(np.uint32)                               # bfloat16: the same rounding on the upper 16 bits
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def sentinel(nbytes):
    """A byte pattern without a short period (and no value the image could not also hold: every byte must be checked)."""
    i = np.arange(nbytes, dtype=np.uint64)
    return ((i * np.uint64(2654435761) >> np.uint64(7)) & np.uint64(0xFF)).astype(np.uint8)


class Destination:
    """raw: the whole buffer as bytes (64-byte aligned start); offset: the element that is (0, 0, 0); strides: (y, x, c)
    in elements.  `before` keeps the sentinel the buffer was filled with."""

    def __init__(self, n_elements, offset, strides, w, h, dtype):
        self.itemsize = np.dtype(STORAGE[dtype]).itemsize
        self.raw = dic.aligned_empty(n_elements * self.itemsize, np.uint8, 0)
        self.raw[...] = sentinel(self.raw.size)
        self.before = self.raw.copy()
        self.offset, self.strides, self.w, self.h, self.dtype = offset, strides, w, h, dtype

    @property
    def address(self):
        return self.raw.ctypes.data + self.offset * self.itemsize

    def image_of(self, raw):
        """The [h][w][3] strided view of the image inside `raw` (a byte buffer of this destination's size)."""
        el = raw.view(STORAGE[self.dtype])
        return np.lib.stride_tricks.as_strided(el[self.offset:], (self.h, self.w, 3), tuple(s * self.itemsize for s in self.strides))

    def expected_raw(self, rgb):
        """The buffer as it must be afterwards: the sentinel, and the emitted image where the image is."""
        exp = self.before.copy()
        self.image_of(exp)[...] = emitted(rgb, self.dtype)
        return exp

    def check(self, rgb, raw=None, what=""):
        raw = self.raw if raw is None else raw
        exp = self.expected_raw(rgb)
        got_img, exp_img = self.image_of(raw), self.image_of(exp)
        same = got_img.view(np.uint8 if self.itemsize == 1 else {2: np.uint16, 4: np.uint32}[self.itemsize]) == \
            exp_img.view(np.uint8 if self.itemsize == 1 else {2: np.uint16, 4: np.uint32}[self.itemsize])
        assert same.all(), (what, "image", self.dtype, self.strides, self.w, self.h, np.argwhere(~same)[:4])
        bad = np.flatnonzero(raw != exp)
        assert bad.size == 0, (what, "outside the image", self.dtype, self.strides, self.w, self.h, bad[:8])


def destination(w, h, dtype, layout):
    base1 = 1 if layout.endswith("_base1") else 0
    kind = layout[:-6] if base1 else layout
    cw, ch = (w + 16 + 15) // 16 * 16, h + 2
    if kind == "HWC":
        return Destination(h * w * 3 + base1 + 5, base1, (3 * w, 3, 1), w, h, dtype)
    if kind == "CHW":
        return Destination(h * w * 3 + base1 + 5, base1, (w, 1, h * w), w, h, dtype)
    if kind == "HWC_crop":
        return Destination(ch * cw * 3 + base1, base1 + (cw + 16) * 3, (3 * cw, 3, 1), w, h, dtype)
    if kind == "CHW_crop":
        return Destination(3 * ch * cw + base1, base1 + cw + 16, (cw, 1, ch * cw), w, h, dtype)
    if kind == "HWC_pitch1":
        return Destination(h * (3 * w + 1) + 5, 0, (3 * w + 1, 3, 1), w, h, dtype)
    assert kind == "WHC"
    return Destination(w * h * 3 + 5, 0, (3, 3 * h, 1), w, h, dtype)


def blocks(w, h, factor=1):
    nb = ((w + 7) // 8) * ((h + 7) // 8)
    nbc = ((w + 8 * factor - 1) // (8 * factor)) * ((h + 8 * factor - 1) // (8 * factor))
    return nb, nbc


def random_coeffs(w, h, factor, seed):
    """Dequantised coefficients in the frame layout of the header: AC in +-1024 thinning out with the frequency, the DC
    spread over its range -- pixels of every level, clamped ones included."""
    rng = np.random.default_rng(seed)
    nb, nbc = blocks(w, h, factor)
    co = np.zeros((nb + 2 * nbc, 64), np.int16)
    k = np.arange(64)
    keep = rng.random(co.shape) < 1.0 / (1.0 + 0.15 * ((k % 8) + (k // 8)) ** 2)
    co[...] = np.where(keep, rng.integers(-1024, 1025, co.shape), 0) // (1 + ((k % 8) + (k // 8)) // 2)
    co[:, 0] = rng.integers(-1024, 1024, co.shape[0])
    return co.reshape(3, nb, 64) if factor == 1 else co


def all_bytes_coeffs(reconstruct):
    """A 128 x 128 4:4:4 frame of flat grey blocks whose pixels take every value 0..255 (one block per value), and those
    pixels: the DC of each level is looked up by `reconstruct` (coeffs, w, h) -> uint8 [h][w][3]."""
    dcs = np.arange(-1100, 1100)
    n = dcs.size
    w = 8 * n
    probe = np.zeros((3, n, 64), np.int16)
    probe[0, :, 0] = dcs
    px = reconstruct(probe, w, 8)
    level = px[0, ::8, 0]
    assert (px == np.repeat(level, 8)[None, :, None]).all()
    co = np.zeros((3, 256, 64), np.int16)
    for v in range(256):
        hit = np.flatnonzero(level == v)
        assert hit.size, v
        co[0, v, 0] = dcs[hit[0]]
    return co, 128, 128


def parse_jpeg_dump(d):
    """The canonical dump of ref_read_jpeg / gzh_read_jpeg (oracle/ref_harness.cc) -> dict."""
    pos = [0]

    def i32():
        v = struct.unpack_from("<i", d, pos[0])[0]
        pos[0] += 4
        return v

    def blob():
        n = i32()
        b = d[pos[0]:pos[0] + n]
        pos[0] += n
        return b
    out = {"w": i32(), "h": i32()}
    comps = [dict(zip(("id", "h_samp", "v_samp", "quant_idx", "wb", "hb"), (i32() for _ in range(6)))) for _ in range(i32())]
    quant = []
    for _ in range(i32()):
        index, precision = i32(), i32()
        quant.append({"index": index, "precision": precision, "values": np.array([i32() for _ in range(64)], np.int32)})
    out["app"] = [blob() for _ in range(i32())]
    out["com"] = [blob() for _ in range(i32())]
    out["tail"] = blob()
    for c in comps:
        n = c["wb"] * c["hb"] * 64
        c["coeffs"] = np.frombuffer(d, np.int16, n, pos[0]).reshape(c["hb"], c["wb"], 64)
        pos[0] += 2 * n
    assert pos[0] == len(d)
    out["components"], out["quant"] = comps, quant
    return out


def frame_of_dump(j):
    """(dequantised coefficients in the frame layout, chroma factor) of a parsed dump, as OutputImage::CopyFromJpegData
    fills an OutputImage: the blocks inside the image's grid, a one-component file with two zero chroma components."""
    w, h = j["w"], j["h"]
    comps = j["components"]
    factor = 1
    if len(comps) == 3 and comps[0]["h_samp"] == 2 * comps[1]["h_samp"]:
        factor = 2
    nb, nbc = blocks(w, h, factor)
    co = np.zeros((nb + 2 * nbc, 64), np.int16)
    first = (0, nb, nb + nbc)
    for i, c in enumerate(comps):
        f = 1 if i == 0 else factor
        bw, bh = (w + 8 * f - 1) // (8 * f), (h + 8 * f - 1) // (8 * f)
        deq = c["coeffs"][:bh, :bw].astype(np.int32) * j["quant"][c["quant_idx"]]["values"]
        assert np.abs(deq).max() < 32768
        co[first[i]:first[i] + bw * bh] = deq.reshape(-1, 64)
    return (co.reshape(3, nb, 64) if factor == 1 else co), factor
