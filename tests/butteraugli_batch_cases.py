"""Shared by tests/test_butteraugli_batch_emu.py (CPU emulation: "device memory" is host memory) and
tests/test_butteraugli_batch_gpu.py (memory of the MI355X): gz_butteraugli_batch, n image pairs through one chain.

Two judges, both for equality of bits: a checker's diffmap of each pair (butteraugli_pair_cases.expected: the CPU
restatement under oracle/, the unmodified reference where it is built), and this library's sequential path -- one
context per reference (gz_create_from_device), gz_compare_device_pixels per pair.

Shapes are the smallest at which the batched indexing can go wrong; every image of a batch has other content, so that
a kernel that reads or writes a neighbour's plane changes a result.  A case takes `mem` (butteraugli_pair_cases)."""
import numpy as np

import butteraugli_pair_cases as bpc
import device_input_cases as dic
import device_output_cases as doc
import fields
import images
from checkers import assert_bits_equal, bits
from guetzli_amd.capi import device_batch, device_image, device_map, device_map_batch

# 8x8: one tile, border paths only; 9x17: crosses the 16-row tile; 67x33: the 64-column tiles, Malta's 32 rows, two
# 16-row tiles; 257x9: k_blur_h's 256 columns; 130x40: several tiles both ways, a pitch that is no multiple of 4
SHAPES = ((8, 8), (9, 17), (67, 33), (257, 9), (130, 40))
BATCH_SIZES = (1, 2, 3, 5, 9)          # at 67x33: workgroup totals that are and are not multiples of 8 (gz_xcd_tile)
DTYPES = dic.DTYPES
IN_LAYOUTS = ("NHWC", "NCHW", "grey", "every_other", "crop", "base1", "same")
MAP_LAYOUTS = ("contiguous", "crop", "transposed")
TARGET = bpc.TARGET
ARENA_PLANES = 43                      # float planes of one image's arena


def arena_bytes(w, h):
    """What one image costs of scratch_cap_bytes: its arena, rounded up to 4 floats, and its result word."""
    return 4 * ((w * h * ARENA_PLANES + 3) // 4 * 4) + 4


_pairs = {}
_canvas = []


def photo_crop(w, h, x0, y0):
    """w x h of the photograph tiled (the photograph itself is 444 x 258)."""
    if not _canvas:
        _canvas.append(images.tiled(1024, 768))
    return np.ascontiguousarray(_canvas[0][y0:y0 + h, x0:x0 + w])


def pairs(w, h, n):
    """(references, distorted) uint8 [n][h][w][3]: the photograph crop against its JPEG round trip, noise against flat, the
    crop against a shifted copy, a constant against another, an image equal to its reference -- then the same kinds again
    with other content."""
    key = (w, h, n)
    if key not in _pairs:
        refs, others = [], []
        for i in range(n):
            kind, k = i % 5, i // 5
            photo = photo_crop(w, h, 120 + 37 * k + 11 * kind, 80 + 23 * k)
            if kind == 0:
                a, b = photo, bpc.decoded_q85(photo)
            elif kind == 1:
                a, b = images.noise(w, h, seed=3 + i), fields.flat(w, h, 128 - 9 * k)
            elif kind == 2:
                a, b = photo, np.ascontiguousarray(np.roll(photo, 1 + k, axis=1))
            elif kind == 3:
                a, b = images.flat(w, h, (60 + i, 90, 120 - i)), images.flat(w, h, (70 + i, 80, 130 - i))
            else:
                a, b = photo, photo.copy()
            refs.append(np.ascontiguousarray(a, np.uint8))
            others.append(np.ascontiguousarray(b, np.uint8))
        _pairs[key] = (np.stack(refs), np.stack(others))
        for a in _pairs[key]:
            a.setflags(write=False)
    return _pairs[key]


def expected(chk, refs, others, broadcast=False):
    """(distances float32 [n], maps float32 [n][h][w]) of the checker; each pair computed once (bpc.expected's cache)."""
    res = [bpc.expected(chk, refs[0 if broadcast else i], others[i]) for i in range(len(others))]
    return np.array([d for d, _ in res], np.float32), np.stack([m for _, m in res])


# ------------------------------------------------------------------ the batches in memory ----
class BatchSource:
    """buf: the flat buffer; offset: its element that is (0, 0, 0, 0); strides: (n, y, x, c) in elements; logical: the
    bytes [n][h][w][3] the ingest rule makes of it."""

    def __init__(self, buf, view, dtype, logical):
        self.buf, self.dtype, self.logical = buf, dtype, logical
        self.itemsize = buf.dtype.itemsize
        self.offset = (view.__array_interface__["data"][0] - buf.__array_interface__["data"][0]) // self.itemsize
        self.strides = tuple(s // self.itemsize for s in view.strides)

    def on(self, mem, stream=0):
        handle = mem.put(self.buf)
        return device_batch(mem.address(handle) + self.offset * self.itemsize, bpc.PIXEL_CODES[self.dtype], self.strides, stream), handle


def lay_out(rgb, dtype, layout):
    """The images `rgb` (uint8 [n][h][w][3]) as elements of `dtype` in a fresh 64-byte aligned buffer: NHWC / NCHW
    contiguous; grey: [n][h][w] with stride_c = 0 (channel 0 counts); every_other: x[::2] of a batch of 2n; crop: views
    inside canvases; base1: one element off alignment; same: ONE image with stride_n = 0 (image 0, n times)."""
    n, h, w, _ = rgb.shape
    st = dic.STORAGE[dtype]
    poison = 0xAB if st != np.float32 else np.float32(np.nan)
    logical = np.array(rgb)
    as_strided = np.lib.stride_tricks.as_strided
    if layout == "NHWC":
        buf = dic.aligned_empty(n * h * w * 3, st, poison)
        view = buf.reshape(n, h, w, 3)
    elif layout == "NCHW":
        buf = dic.aligned_empty(n * h * w * 3, st, poison)
        view = buf.reshape(n, 3, h, w).transpose(0, 2, 3, 1)
    elif layout == "grey":
        buf = dic.aligned_empty(n * h * w, st, poison)
        g = buf.reshape(n, h, w)
        view = as_strided(g, (n, h, w, 3), g.strides + (0,))
        logical = np.repeat(logical[..., :1], 3, axis=-1)
    elif layout == "every_other":
        buf = dic.aligned_empty(2 * n * h * w * 3, st, poison)
        view = buf.reshape(2 * n, h, w, 3)[::2]
    elif layout == "crop":
        cw, ch = (w + 16 + 15) // 16 * 16, h + 2
        buf = dic.aligned_empty(n * ch * cw * 3, st, poison)
        view = buf.reshape(n, ch, cw, 3)[:, 1:1 + h, 16:16 + w]
    elif layout == "base1":
        buf = dic.aligned_empty(n * h * w * 3 + 1, st, poison)
        view = buf[1:].reshape(n, h, w, 3)
    else:
        assert layout == "same"
        buf = dic.aligned_empty(h * w * 3, st, poison)
        one = buf.reshape(h, w, 3)
        view = as_strided(one, (n, h, w, 3), (0,) + one.strides)
        logical = np.repeat(logical[:1], n, axis=0)
    if layout == "grey":
        buf.reshape(n, h, w)[...] = dic.from_bytes(logical[..., 0], dtype)
    elif layout == "same":
        buf.reshape(h, w, 3)[...] = dic.from_bytes(logical[0], dtype)
    else:
        view[...] = dic.from_bytes(logical, dtype)
    return BatchSource(buf, view, dtype, logical)


class MapBatchDestination:
    """n maps inside a sentinel buffer: raw = the whole buffer as bytes; view_of(raw) = the [n][h][w] elements."""

    def __init__(self, n, w, h, dtype, layout):
        self.dtype, self.shape = dtype, (n, h, w)
        st = bpc.MAP_STORAGE[dtype]
        self.itemsize = np.dtype(st).itemsize
        if layout == "contiguous":
            count, make = n * h * w + 5, lambda el: el[:n * h * w].reshape(n, h, w)
        elif layout == "crop":
            cw, ch = (w + 16 + 15) // 16 * 16, h + 2
            count, make = n * ch * cw, lambda el: el.reshape(n, ch, cw)[:, 1:1 + h, 16:16 + w]
        else:
            assert layout == "transposed"
            count, make = w * n * h + 5, lambda el: el[:w * n * h].reshape(w, n, h).transpose(1, 2, 0)
        self.make = make
        self.raw = dic.aligned_empty(count * self.itemsize, np.uint8, 0)
        self.raw[...] = doc.sentinel(self.raw.size)
        self.before = self.raw.copy()
        view = self.view_of(self.raw)
        self.offset = (view.__array_interface__["data"][0] - self.raw.__array_interface__["data"][0]) // self.itemsize
        self.strides = tuple(s // self.itemsize for s in view.strides)

    def view_of(self, raw):
        return self.make(raw.view({2: np.uint16, 4: np.uint32}[self.itemsize]))

    def on(self, mem, stream=0):
        handle = mem.put(self.raw)
        return device_map_batch(mem.address(handle) + self.offset * self.itemsize, bpc.MAP_CODES[self.dtype], self.strides, stream), handle

    def check(self, maps, raw, what=""):
        """Every element is the value rule's of the float32 `maps`, every byte outside the n*h*w elements the sentinel."""
        exp = self.before.copy()
        want = bpc.emitted_map(maps, self.dtype)
        self.view_of(exp)[...] = want.view(np.uint32) if self.itemsize == 4 else want
        got_img, exp_img = self.view_of(raw), self.view_of(exp)
        same = got_img == exp_img
        assert same.all(), (what, "maps", self.dtype, self.strides, np.argwhere(~same)[:4], got_img[~same][:4], exp_img[~same][:4])
        bad = np.flatnonzero(raw != exp)
        assert bad.size == 0, (what, "outside the maps", self.dtype, self.strides, bad[:8])


DIST_PAD = 3   # the distances start this many floats into their sentinel buffer: 4-byte aligned, not 16


def run_batch(L, mem, ref, other, w, h, n, n_ref=None, maps=None, scratch_bytes=0, streams=(0, 0)):
    """gz_butteraugli_batch of two BatchSources -> (distances float32 [n], float32 maps [n][h][w] or None).  The device's
    distances sit inside a sentinel buffer, which is checked, and equal the host copy; so are the maps' surroundings."""
    rb, rheld = ref.on(mem, streams[0])
    ob, oheld = other.on(mem, streams[0])
    dbuf = np.frombuffer(doc.sentinel(4 * (n + 2 * DIST_PAD)).tobytes(), np.float32).copy()
    dhandle = mem.put(dbuf)
    mb, mhandle = maps.on(mem, streams[1]) if maps is not None else (None, None)
    host = L.butteraugli_batch(rb, ob, w, h, n, mem.address(dhandle) + 4 * DIST_PAD, n_ref=n_ref, maps=mb, scratch_bytes=scratch_bytes)
    got = np.array(mem.get(dhandle))
    assert np.array_equal(got[:DIST_PAD].view(np.uint32), dbuf[:DIST_PAD].view(np.uint32)), "in front of the distances"
    assert np.array_equal(got[DIST_PAD + n:].view(np.uint32), dbuf[DIST_PAD + n:].view(np.uint32)), "behind the distances"
    dev = got[DIST_PAD:DIST_PAD + n]
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32)), (dev, host)
    out = None
    if maps is not None:
        raw = np.array(mem.get(mhandle))
        out = np.ascontiguousarray(bpc.widen_map(np.ascontiguousarray(maps.view_of(raw)), maps.dtype)).reshape(n, h, w)
        if maps.dtype == "float32":
            maps.check(out, raw, "around the maps")
    del rheld, oheld
    return dev.copy(), out


def sequential(L, mem, refs, others, broadcast=False):
    """The library's own judge: one context per reference (one warm context when it is broadcast), one
    gz_compare_device_pixels per pair -> (distances, maps)."""
    n, h, w, _ = others.shape
    ds, ms = [], []
    ctx = None
    for i in range(n):
        if ctx is None or not broadcast:
            if ctx is not None:
                ctx.close()
            src = dic.lay_out(refs[0 if broadcast else i], "uint8", "HWC")
            held = mem.put(src.storage)
            ctx = L.context_from_device(device_image(mem.address(held) + src.offset, 0, src.strides), w, h, TARGET)
        d, m = bpc.compare_pixels(ctx, mem, dic.lay_out(others[i], "uint8", "HWC"), w, h)
        ds.append(d)
        ms.append(m)
    ctx.close()
    return np.array(ds, np.float32), np.stack(ms)


def assert_batch_equal(got, exp, what):
    (gd, gm), (ed, em) = got, exp
    assert np.array_equal(gd.view(np.uint32), ed.view(np.uint32)), (what, "distances", gd, ed)
    if gm is not None:
        for i in range(len(em)):
            assert_bits_equal(gm[i], em[i], f"{what}: map {i}")


# ------------------------------------------------------------------ cases ----
def case_parity(L, mem, chk, w, h, n):
    """Distances and float32 maps of n distinct pairs: the checker's and the sequential path's bits."""
    refs, others = pairs(w, h, n)
    got = run_batch(L, mem, lay_out(refs, "uint8", "NHWC"), lay_out(others, "uint8", "NHWC"), w, h, n,
                    maps=MapBatchDestination(n, w, h, "float32", "contiguous"))
    assert_batch_equal(got, expected(chk, refs, others), f"{n} x {w}x{h} against {chk.name}")
    assert_batch_equal(got, sequential(L, mem, refs, others), f"{n} x {w}x{h} against the sequential path")
    d_only, none = run_batch(L, mem, lay_out(refs, "uint8", "NHWC"), lay_out(others, "uint8", "NHWC"), w, h, n)
    assert none is None and np.array_equal(d_only.view(np.uint32), got[0].view(np.uint32)), "without maps"


def case_broadcast(L, mem, chk, w, h, n):
    """ONE reference against n images: n calls on one warm context."""
    refs, others = pairs(w, h, n)
    one = lay_out(refs[:1], "uint8", "NHWC")
    got = run_batch(L, mem, one, lay_out(others, "uint8", "NHWC"), w, h, n, n_ref=1, maps=MapBatchDestination(n, w, h, "float32", "contiguous"))
    assert_batch_equal(got, expected(chk, refs, others, broadcast=True), f"broadcast {n} x {w}x{h} against {chk.name}")
    assert_batch_equal(got, sequential(L, mem, refs, others, broadcast=True), f"broadcast {n} x {w}x{h} against one warm context")


def case_way_in(L, mem, chk, dtype, layout, w=67, h=33, n=3):
    """Every element type and batch layout, for both batches: the bytes the layout holds decide."""
    refs, others = pairs(w, h, n)
    rs, os_ = lay_out(refs, dtype, layout), lay_out(others, dtype, layout)
    got = run_batch(L, mem, rs, os_, w, h, n, maps=MapBatchDestination(n, w, h, "float32", "contiguous"))
    assert_batch_equal(got, expected(chk, rs.logical, os_.logical), f"{dtype} {layout}")
    if layout == "same":   # the same image n times: n equal results
        assert len(set(got[0].view(np.uint32).tolist())) == 1
        assert all(np.array_equal(got[1][0], got[1][i]) for i in range(n))


def case_maps(L, mem, chk, dtype, layout, w=67, h=33, n=3):
    """Maps of every element type into every layout; the canvas around the n*h*w elements keeps its sentinel."""
    refs, others = pairs(w, h, n)
    ed, em = expected(chk, refs, others)
    dest = MapBatchDestination(n, w, h, dtype, layout)
    rb, rheld = lay_out(refs, "uint8", "NHWC").on(mem)
    ob, oheld = lay_out(others, "uint8", "NHWC").on(mem)
    dist = mem.put(np.zeros(n, np.float32))
    mb, handle = dest.on(mem)
    host = L.butteraugli_batch(rb, ob, w, h, n, mem.address(dist), maps=mb)
    assert np.array_equal(host.view(np.uint32), ed.view(np.uint32))
    dest.check(em, np.array(mem.get(handle)), f"{dtype} {layout}")


def case_chunking(L, mem, w=67, h=33, n=5):
    """A cap of two images' scratch: 2 + 2 + 1, the unchunked bits -> the distances and maps of both runs."""
    refs, others = pairs(w, h, n)
    args = lambda: (lay_out(refs, "uint8", "NHWC"), lay_out(others, "uint8", "NHWC"), w, h, n)
    whole = run_batch(L, mem, *args(), maps=MapBatchDestination(n, w, h, "float32", "crop"))
    chunked = run_batch(L, mem, *args(), maps=MapBatchDestination(n, w, h, "float32", "crop"), scratch_bytes=2 * arena_bytes(w, h) + 64)
    assert_batch_equal(chunked, whole, "chunked against whole")
    one = lay_out(refs[:1], "uint8", "NHWC")
    b_whole = run_batch(L, mem, one, args()[1], w, h, n, n_ref=1, maps=MapBatchDestination(n, w, h, "float32", "contiguous"))
    b_chunked = run_batch(L, mem, one, args()[1], w, h, n, n_ref=1, maps=MapBatchDestination(n, w, h, "float32", "contiguous"),
                          scratch_bytes=2 * arena_bytes(w, h) + 64)
    assert_batch_equal(b_chunked, b_whole, "broadcast, chunked against whole")
    return whole
