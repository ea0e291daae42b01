"""Shared by tests/test_butteraugli_pair_emu.py (CPU emulation: "device memory" is host memory) and
tests/test_butteraugli_pair_gpu.py (memory of the MI355X): the image-pair metric -- gz_compare_device_pixels,
gz_compare_rgb, gz_distmap_device, and the map's emit kernel alone through gz_probe_emit_map.

What judges the results: a checker's diffmap(rgb0, rgb1) -- the CPU restatement under oracle/, and the unmodified
reference where it is built -- of the linear planes float32(srgb_to_linear_table()[byte]) of each image's bytes, the bytes
taken by the numpy rules of device_input_cases / device_alpha_cases.  Every comparison is bitwise.

A case takes `mem`, which says where device memory is: HostMemory here (numpy buffers are the device's memory in the
emulation), the GPU suite's own for torch tensors."""
import numpy as np

import device_alpha_cases as dac
import device_input_cases as dic
import device_output_cases as doc
import fields
import images
from checkers import assert_bits_equal, bits, oracle
from guetzli_amd.capi import GZ_DT_BF16, GZ_DT_F16, GZ_DT_F32, GuetzliAmdError, device_map, device_pixels

WIDTHS = (8, 9, 15, 16, 17, 33, 61, 64, 67)
HEIGHTS = (8, 9, 17)
SIZES = tuple((w, h) for h in HEIGHTS for w in WIDTHS)
TARGET = 0.971769
MAP_DTYPES = ("float32", "float16", "bfloat16")
MAP_CODES = {"float32": GZ_DT_F32, "float16": GZ_DT_F16, "bfloat16": GZ_DT_BF16}
MAP_STORAGE = {"float32": np.float32, "float16": np.uint16, "bfloat16": np.uint16}
PIXEL_CODES = {"uint8": 0, "float32": 1, "float16": 2, "bfloat16": 3, "uint16": 4}
# contiguous; crop: a view inside a canvas whose pitch keeps the 16-byte stores open; base1: one element further on (the
# base address is not 16-byte aligned); pitch1: a row pitch that is no multiple of 16 bytes; transposed: x outermost
MAP_LAYOUTS = ("contiguous", "crop", "base1", "pitch1", "transposed")
PAIRS = ("photo", "noise_flat", "self", "shift")
BACKGROUND = (3, 200, 77)

# the Annex K tables at quality 85 (libjpeg's scaling: (base * 30 + 50) / 100), luminance and chrominance
_K1 = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
                100, 103, 99])
_K2 = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
               + [99] * 32)
Q85 = np.stack([np.maximum((t * 30 + 50) // 100, 1) for t in (_K1, _K2, _K2)]).astype(np.int32)


class HostMemory:
    """Device memory of the emulation: the numpy buffer itself."""

    def put(self, array):
        return array

    def address(self, handle):
        return handle.ctypes.data

    def get(self, handle):
        return handle


def decoded_q85(rgb):
    """The pixels of the image after a JPEG round trip at quality 85 (the checker's own transform and decode)."""
    h, w, _ = rgb.shape
    return oracle.reconstruct(oracle.encode_rgb(rgb), w, h, Q85)[1]


_pairs = {}


def pair(name, w, h):
    """(reference, distorted) uint8 [h][w][3] of the field pair `name`."""
    key = (name, w, h)
    if key not in _pairs:
        photo = images.crop(w, h, 120, 80)
        _pairs[key] = {"photo": lambda: (photo, decoded_q85(photo)),
                       "noise_flat": lambda: (fields.noise(w, h), fields.flat(w, h, 128)),
                       "self": lambda: (photo, photo.copy()),
                       "shift": lambda: (photo, np.ascontiguousarray(np.roll(photo, 1, axis=1)))}[name]()
    return _pairs[key]


_expected = {}


def expected(chk, rgb0, rgb1):
    """(distance as the float the library returns, float32 map) of the checker for the two images' bytes; computed once
    per checker and pair of images, and handed out read-only."""
    key = (chk.name, rgb0.shape, rgb0.tobytes(), rgb1.tobytes())
    if key not in _expected:
        d, s = chk.diffmap(fields.linear(rgb0), fields.linear(rgb1))
        d.setflags(write=False)
        _expected[key] = (np.float32(s), d)
    return _expected[key]


def block_maxima(dm):
    h, w = dm.shape
    bw, bh = (w + 7) // 8, (h + 7) // 8
    pad = np.zeros((bh * 8, bw * 8), np.float32)
    pad[:h, :w] = dm
    return pad.reshape(bh, 8, bw, 8).max(axis=(1, 3)).reshape(-1)


# ------------------------------------------------------------------ sources ----
def pixels_of(mem, src, stream=0, background=(0, 0, 0)):
    """(capi.GzDevicePixels, what keeps the memory alive) of a device_input_cases / device_alpha_cases Source."""
    held = [mem.put(src.storage)]
    base = mem.address(held[0])
    alpha = 0
    if getattr(src, "alpha_storage", None) is not None:
        if src.alpha_storage is src.storage:
            abase = base
        else:
            held.append(mem.put(src.alpha_storage))
            abase = mem.address(held[1])
        alpha = abase + src.alpha_offset * src.itemsize
    px = device_pixels(base + src.offset * src.itemsize, PIXEL_CODES[src.dtype], src.strides, stream, alpha, background)
    return px, held


def storage_of_bytes(rgb, dtype):
    """Storage [h][w][3] of `dtype` whose bytes, by the ingest rule, are `rgb` (uint16: the byte on top of low bits)."""
    if dtype == "uint16":
        low = images.noise(rgb.shape[1], rgb.shape[0], seed=3).astype(np.uint16)
        return (rgb.astype(np.uint16) << np.uint16(8)) | low
    return dic.from_bytes(rgb, dtype)


# ------------------------------------------------------------------ map destinations ----
def emitted_map(plane, dtype):
    """The value rule of gz_device_map: the storage elements of the float32 `plane`."""
    f = np.ascontiguousarray(plane, np.float32)
    if dtype == "float32":
        return f
    if dtype == "float16":
        with np.errstate(all="ignore"):
            return f.astype(np.float16).view(np.uint16)     # numpy rounds to nearest, ties to even
    u = f.view(np.uint32)                                   # bfloat16: device_output_cases.emitted's rule
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


class MapDestination:
    """device_output_cases.Destination for a 2-D image: raw = the whole buffer as bytes (64-byte aligned, filled with
    its sentinel), offset = the element that is (0, 0), strides = (y, x) in elements."""

    def __init__(self, n_elements, offset, strides, w, h, dtype):
        self.itemsize = np.dtype(MAP_STORAGE[dtype]).itemsize
        self.raw = dic.aligned_empty(n_elements * self.itemsize, np.uint8, 0)
        self.raw[...] = doc.sentinel(self.raw.size)
        self.before = self.raw.copy()
        self.offset, self.strides, self.w, self.h, self.dtype = offset, strides, w, h, dtype

    def image_of(self, raw):
        el = raw.view({2: np.uint16, 4: np.uint32}[self.itemsize])
        return np.lib.stride_tricks.as_strided(el[self.offset:], (self.h, self.w), tuple(s * self.itemsize for s in self.strides))

    def on(self, mem, stream=0):
        """(capi.GzDeviceMap, the handle of the buffer in device memory)."""
        handle = mem.put(self.raw)
        return device_map(mem.address(handle) + self.offset * self.itemsize, MAP_CODES[self.dtype], self.strides, stream), handle

    def check(self, plane, raw, what="", nan_is_nan=False):
        """Every element of the image is the rule's, every byte outside it the sentinel."""
        exp = self.before.copy()
        want = emitted_map(plane, self.dtype)
        self.image_of(exp)[...] = want.view(np.uint32) if self.itemsize == 4 else want
        got_img, exp_img = self.image_of(raw), self.image_of(exp)
        same = got_img == exp_img
        if nan_is_nan:
            nan = np.isnan(np.asarray(plane, np.float32))
            same = np.where(nan, np.isnan(widen_map(got_img, self.dtype)), same)
            self.image_of(exp)[nan] = got_img[nan]
        assert same.all(), (what, "image", self.dtype, self.strides, self.w, self.h, np.argwhere(~same)[:4],
                            got_img[~same][:4], exp_img[~same][:4])
        bad = np.flatnonzero(raw != exp)
        assert bad.size == 0, (what, "outside the image", self.dtype, self.strides, self.w, self.h, bad[:8])


def widen_map(storage, dtype):
    if dtype == "float32":
        return np.ascontiguousarray(storage).view(np.float32)
    if dtype == "float16":
        return np.ascontiguousarray(storage).view(np.float16).astype(np.float32)
    return (np.ascontiguousarray(storage).astype(np.uint32) << np.uint32(16)).view(np.float32)


def map_destination(w, h, dtype, layout):
    cw, ch = (w + 16 + 15) // 16 * 16, h + 2
    if layout == "contiguous":
        return MapDestination(h * w + 5, 0, (w, 1), w, h, dtype)
    if layout == "crop":
        return MapDestination(ch * cw, cw + 16, (cw, 1), w, h, dtype)
    if layout == "base1":
        return MapDestination(h * w + 6, 1, (w, 1), w, h, dtype)
    if layout == "pitch1":
        p = w + 1 if (w + 1) % 4 else w + 2      # (rows of p elements: p * itemsize is no multiple of 16)
        return MapDestination(h * p + 5, 0, (p, 1), w, h, dtype)
    assert layout == "transposed"
    return MapDestination(w * h + 5, 0, (1, h), w, h, dtype)


def plane_of_distances(w, h, seed):
    """Floats a distance map holds: mostly 0 .. 30, a few tiny ones (float16 subnormals) and exact zeros."""
    rng = np.random.default_rng(seed)
    p = (rng.random((h, w)) * 30).astype(np.float32)
    p[rng.random((h, w)) < 0.1] = np.float32(1e-6)
    p[rng.random((h, w)) < 0.05] = 0
    return p


def rounding_plane():
    """float32 [256][512]: every non-negative finite float16 value v, and for each v the float32 values just below, at
    and just above the midpoint to its successor (for the largest: to 65536, so into overflow); the neighbourhood of
    float16's maximum; the bfloat16 ties; sign-flipped samples; +-inf and NaN."""
    v = np.arange(0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)
    succ = np.append(v[1:], np.float32(65536))
    mid = ((v.astype(np.float64) + succ) / 2).astype(np.float32)
    assert (mid.astype(np.float64) * 2 == v.astype(np.float64) + succ).all()       # the midpoints are float32 values
    inf = np.float32(np.inf)
    parts = [v, np.nextafter(mid, -inf), mid, np.nextafter(mid, inf)]
    top = np.float32(65504)
    special = [top, np.nextafter(top, inf), 65519.996, 65520, np.nextafter(np.float32(65520), inf), 65536, 1e5, 1e38,
               np.finfo(np.float32).max, np.inf, -np.inf, np.nan, -np.nan, 1e-6, 2.0 ** -24, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), inf),
               1e-45, 2.0 ** -14, np.nextafter(np.float32(2.0 ** -14), -inf), -0.0]
    with np.errstate(all="ignore"):
        parts.append(np.array(special, np.float32))
    rng = np.random.default_rng(20261019)
    hi = rng.integers(0, 0x7F80, 1000, dtype=np.uint64).astype(np.uint32) << np.uint32(16)   # finite, non-negative
    parts += [(hi | np.uint32(low)).view(np.float32) for low in (0x7FFF, 0x8000, 0x8001)]
    parts.append(-np.concatenate(parts)[rng.integers(0, 4 * v.size, 1000)])
    flat = np.concatenate(parts).astype(np.float32)
    assert flat.size <= 512 * 256
    return np.ascontiguousarray(np.resize(flat, 512 * 256).reshape(256, 512))


# ------------------------------------------------------------------ cases ----
def compare_pixels(ctx, mem, src, w, h, dtype="float32", layout="contiguous", background=(0, 0, 0)):
    """gz_compare_device_pixels of a Source with a map destination -> (distance, float32 map); the destination's
    surroundings are checked too."""
    px, held = pixels_of(mem, src, background=background)
    dest = map_destination(w, h, dtype, layout)
    dm, handle = dest.on(mem)
    d = ctx.compare_device_pixels(px, dm)
    raw = mem.get(handle)
    got = np.ascontiguousarray(widen_map(dest.image_of(raw), dtype))
    dest.check(got, raw, what="around the map", nan_is_nan=True)   # (the image is the caller's to judge: the sentinel here)
    del held
    return np.float32(d), got


def check_pair(L, mem, chk, rgb0, rgb1, what, layout="contiguous"):
    """compare_device_pixels (u8 HWC) and compare_rgb of rgb1 against a context of rgb0: the checker's bits."""
    h, w, _ = rgb0.shape
    ed, em = expected(chk, rgb0, rgb1)
    with L.context(rgb0, TARGET) as ctx:
        d, m = compare_pixels(ctx, mem, dic.lay_out(rgb1, "uint8", "HWC"), w, h, layout=layout)
        assert_bits_equal(m, em, f"map of {what}")
        assert bits(d) == bits(ed), (what, d, ed)
        d2, m2 = ctx.compare_rgb(rgb1)
        assert_bits_equal(m2, em, f"compare_rgb map of {what}")
        assert bits(np.float32(d2)) == bits(ed), (what, d2, ed)
        assert bits(np.float32(ctx.compare_rgb(rgb1, want_distmap=False)[0])) == bits(ed)
        px, held = pixels_of(mem, dic.lay_out(rgb1, "uint8", "HWC"))
        assert bits(np.float32(ctx.compare_device_pixels(px))) == bits(ed)


def case_pair_parity_every_size(L, mem, chk):
    for w, h in SIZES:
        rgb0, rgb1 = pair("photo", w, h)
        check_pair(L, mem, chk, rgb0, rgb1, f"photo {w}x{h}", layout=("contiguous", "crop", "base1")[(w + h) % 3])


def case_pair_parity_every_pair(L, mem, chk):
    for w, h in ((33, 17), (61, 9)):
        for name in PAIRS:
            rgb0, rgb1 = pair(name, w, h)
            check_pair(L, mem, chk, rgb0, rgb1, f"{name} {w}x{h}")
            check_pair(L, mem, chk, rgb1, rgb0, f"{name} {w}x{h} swapped")
        # the metric is not symmetric: the swapped photo pair has a map of its own
        a, b = pair("photo", w, h)
        assert not np.array_equal(expected(chk, a, b)[1], expected(chk, b, a)[1])


WAYS_IN = ("HWC", "CHW", "HWC_crop", "CHW_crop", "HWC_base1", "CHW_crop_base1")


def case_every_way_in(L, mem, chk, dtype):
    """`other` as every layout of `dtype`, then with alpha over a background that is not black."""
    for w, h in ((17, 9), (64, 8)):
        rgb0, rgb1 = pair("photo", w, h)
        ed, em = expected(chk, rgb0, rgb1)
        storage = storage_of_bytes(rgb1, dtype)
        assert np.array_equal(dac.expected_rgb(storage, None, dtype), rgb1)
        rng = np.random.default_rng(w)
        colour = storage_of_bytes(images.noise(w, h, seed=5), dtype)
        alpha = dac.random_alpha(dtype, w * h, rng).reshape(h, w)
        with L.context(rgb0, TARGET) as ctx:
            for layout in WAYS_IN:
                d, m = compare_pixels(ctx, mem, dac.lay_out_opaque(storage, dtype, layout), w, h)
                assert_bits_equal(m, em, f"{dtype} {layout} {w}x{h}")
                assert bits(d) == bits(ed), (dtype, layout, d, ed)
            for layout in ("HWC_rgba", "CHW_rgba_crop", "alpha_apart_base1"):
                src = dac.lay_out(colour, alpha, dtype, layout)
                blended = src.expected(BACKGROUND)
                bd, bm = expected(chk, rgb0, blended)
                d, m = compare_pixels(ctx, mem, src, w, h, background=BACKGROUND)
                assert_bits_equal(m, bm, f"{dtype} {layout} {w}x{h} over {BACKGROUND}")
                assert bits(d) == bits(bd), (dtype, layout, d, bd)


def case_map_emit_alone(L, mem, dtype, layout):
    """gz_probe_emit_map over every width x height: the rule's elements, untouched surroundings."""
    for w, h in SIZES:
        plane = plane_of_distances(w, h, seed=100 * h + w)
        dest = map_destination(w, h, dtype, layout)
        dm, handle = dest.on(mem)
        L.probe_emit_map(plane, dm)
        dest.check(plane, mem.get(handle), what=layout)


def case_rounding(L, mem, dtype):
    plane = rounding_plane()
    h, w = plane.shape
    for layout in ("contiguous", "base1"):      # the 16-byte stores, and element by element
        dest = map_destination(w, h, dtype, layout)
        dm, handle = dest.on(mem)
        L.probe_emit_map(plane, dm)
        dest.check(plane, mem.get(handle), what=("rounding", layout), nan_is_nan=True)


Q = np.full((3, 64), 3, np.int32)
CONFIGS = (dict(patch_reconstruct=2, opsin_ahead=1), dict(single_stream=0), dict(single_stream=1))


def _candidate_context(L, rgb0, config, frame):
    ctx = L.context(rgb0, TARGET)
    ctx.set_config(**config)
    ctx.encode_rgb(download=False)
    if frame == 2:
        ctx.downsample(download=False)
    return ctx


def _fresh_compare(L, rgb0, config, frame, coeffs):
    with _candidate_context(L, rgb0, config, frame) as fresh:
        fresh.set_coeffs(coeffs)
        return fresh.compare()


def _assert_compare_equal(got, exp, what):
    for g, e, name in zip(got, exp, ("distance", "distance map", "block maxima")):
        assert_bits_equal(np.asarray(g, np.float32), np.asarray(e, np.float32), f"{name}: {what}")


def case_state(L, mem, chk, config, frame):
    """A pixel comparison between coefficient comparisons, three times over: the candidate's Compare stays a fresh
    context's, the block weights speak of the pixel pair, gz_encode_rgb returns what it returned."""
    w, h = 33, 17
    rgb0, rgb1 = pair("photo", w, h)
    others = (rgb1, pair("noise_flat", w, h)[0], pair("shift", w, h)[1])
    oc = chk.comparator(rgb0, TARGET)
    with _candidate_context(L, rgb0, config, frame) as ctx:
        first = ctx.encode_rgb()
        if frame == 2:
            ctx.downsample(download=False)
        for k, other in enumerate(others):
            ctx.quantize(np.full((3, 64), 2 + 2 * k, np.int32), download=False)
            cq = ctx.get_coeffs()
            exp = _fresh_compare(L, rgb0, config, frame, cq)
            _assert_compare_equal(ctx.compare(), exp, f"before, round {k}")
            ed, em = expected(chk, rgb0, other)
            d, m = compare_pixels(ctx, mem, dic.lay_out(other, "uint8", "HWC"), w, h)
            assert_bits_equal(m, em, f"pixel map, round {k}")
            assert bits(d) == bits(ed)
            for direction in (1, -1):
                assert_bits_equal(ctx.block_weights(direction, 2, 1.0), oc.block_weights(direction, 2, 1.0, em), f"block weights, round {k}")
            assert ctx.frame_layout()[0] == frame
            assert np.array_equal(ctx.get_coeffs(), cq)
            _assert_compare_equal(ctx.compare(), exp, f"after, round {k}")
            _assert_compare_equal(ctx.compare(), exp, f"after, again, round {k}")   # (on patched planes, where the config keeps them)
            d2, _ = ctx.compare_rgb(other, want_distmap=False)
            assert bits(np.float32(d2)) == bits(ed)
            _assert_compare_equal(ctx.compare(), exp, f"after compare_rgb, round {k}")
        assert np.array_equal(ctx.encode_rgb(), first)
    oc.close()


def case_distmap_device(L, mem):
    """gz_distmap_device: the map of the last comparison that stored one, GZ_E_STATE where none did."""
    w, h = 33, 17
    rgb0, rgb1 = pair("photo", w, h)

    def emitted_now(ctx, dtype="float32", layout="crop"):
        dest = map_destination(w, h, dtype, layout)
        dm, handle = dest.on(mem)
        ctx.distmap_device(dm)
        return dest, mem.get(handle)

    def refused(ctx):
        dest = map_destination(w, h, "float32", "contiguous")
        dm, handle = dest.on(mem)
        try:
            ctx.distmap_device(dm)
        except GuetzliAmdError as e:
            assert "GZ_E_STATE" in str(e)
            assert np.array_equal(mem.get(handle), dest.before)
            return True
        return False

    with L.context(rgb0, TARGET) as ctx:
        assert refused(ctx)                                    # nothing compared yet
        ctx.encode_rgb(download=False)
        ctx.quantize(Q, download=False)
        _, dm, _ = ctx.compare()                               # gz_compare(distmap != NULL)
        for dtype in MAP_DTYPES:
            dest, raw = emitted_now(ctx, dtype)
            dest.check(dm, raw, what="after gz_compare")
        ctx.compare(want_distmap=False)
        assert refused(ctx)                                    # the last comparison stored none
        px, held = pixels_of(mem, dic.lay_out(rgb1, "uint8", "HWC"))
        ctx.compare_device_pixels(px)
        assert refused(ctx)
        _, pm = ctx.compare_rgb(rgb1)
        dest, raw = emitted_now(ctx)
        dest.check(pm, raw, what="after gz_compare_rgb")
        ctx.compare_begin()
        ctx.compare_end()
        assert refused(ctx)
        ctx.set_config(store_distmap=1)
        ctx.compare(want_distmap=False)                        # any comparison under store_distmap
        dest, raw = emitted_now(ctx, "bfloat16", "transposed")
        dest.check(dm, raw, what="under store_distmap")
        ctx.compare_begin()
        ctx.compare_end()
        dest, raw = emitted_now(ctx)
        dest.check(dm, raw, what="gz_compare_end under store_distmap")
        ctx.set_rgb(rgb0)
        assert refused(ctx)                                    # a new original: the plane was its scratch


def case_pending_compare_refuses(L, mem):
    w, h = 33, 17
    rgb0, rgb1 = pair("photo", w, h)
    with L.context(rgb0, TARGET) as ctx:
        ctx.encode_rgb(download=False)
        ctx.quantize(Q, download=False)
        exp = ctx.compare()
        px, held = pixels_of(mem, dic.lay_out(rgb1, "uint8", "HWC"))
        ctx.compare_begin()
        for call in (lambda: ctx.compare_device_pixels(px), lambda: ctx.compare_rgb(rgb1)):
            try:
                call()
                raise AssertionError("a pixel comparison ran inside gz_compare_begin .. gz_compare_end")
            except GuetzliAmdError as e:
                assert "GZ_E_STATE" in str(e)
        assert bits(np.float32(ctx.compare_end())) == bits(np.float32(exp[0]))
        assert bits(np.float32(ctx.compare_device_pixels(px))) == bits(expected(oracle, rgb0, rgb1)[0])
