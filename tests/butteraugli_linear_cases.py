"""Shared by tests/test_butteraugli_linear_emu.py (CPU emulation: "device memory" is host memory) and
tests/test_butteraugli_linear_gpu.py (memory of the MI355X): butteraugli of LINEAR float images -- gz_create_from_device_linear,
gz_set_linear_device, gz_compare_device_linear, gz_butteraugli_linear, and the ingest kernel's planes through
gz_probe_linear_planes.

What judges the results: a checker's diffmap(rgb0, rgb1) -- the CPU restatement under oracle/, and the unmodified
reference where it is built -- of the float32 planes numpy's exact widening (times the scale, in float32) makes of each
image's elements.  Every comparison is bitwise.

A case takes `mem`, which says where device memory is (butteraugli_pair_cases.HostMemory here, the GPU suite's own for
torch tensors)."""
import numpy as np

import butteraugli_pair_cases as bpc
import device_input_cases as dic
import device_output_cases as doc
import fields
import heatmap_cases as hc
import images
from checkers import assert_bits_equal, bits, oracle
from guetzli_amd.capi import GuetzliAmdError, device_pixels

DTYPES = ("float32", "float16", "bfloat16")
PARITY_SIZES = ((8, 8), (9, 15), (33, 17), (64, 48))
SMALL_SIZES = ((1, 1), (3, 5), (7, 9), (9, 7), (4, 40))
# HWC / CHW contiguous: the interleaved and the planar 16-byte reads where the width allows them; *_base1 crops: the
# image starts at an odd element of a larger canvas, so the base is not 16-byte aligned -- element by element; grey:
# [h][w] with stride_c == 0 (planar reads of one plane three times)
LAYOUTS = ("HWC", "CHW", "HWC_crop_base1", "CHW_crop_base1", "grey")
# w % P in {0, 1, P - 1} for P = 4 (float32) and P = 8 (the 16-bit types); all of them leave rows whose stores start off
# the 16-byte grid (the planes' pitch is w)
WIDTHS = {"float32": (8, 9, 11, 16), "float16": (8, 9, 15, 16), "bfloat16": (8, 9, 15, 16)}
TARGET = bpc.TARGET


# ------------------------------------------------------------------ elements and planes ----
def to_storage(values, dtype):
    """float32 values -> storage elements of `dtype` (device_input_cases: float32, or the 16 bits of the others),
    rounded to nearest even where the type is narrower."""
    v = np.ascontiguousarray(values, np.float32)
    if dtype == "float32":
        return v.copy()
    if dtype == "float16":
        with np.errstate(all="ignore"):
            return v.astype(np.float16).view(np.uint16)
    u = v.view(np.uint32)
    nan = np.isnan(v)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return np.where(nan, ((u >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16), r)


def rule(storage, dtype, scale=1.0):
    """The value rule restated: (float32 values, number of elements it altered) of storage elements.
      v = x.astype(f32) * f32(scale);  np.where(np.isnan(v) | (v < 0), 0, np.where(v > 255, 255, v))"""
    with np.errstate(all="ignore"):
        v = dic.widen(storage, dtype) * np.float32(scale)
        assert v.dtype == np.float32
        low = np.isnan(v) | (v < 0)
        high = v > 255
        out = np.where(low, np.float32(0), np.where(high, np.float32(255), v)).astype(np.float32)
    return out, int(low.sum() + high.sum())


def planes_of(logical, dtype, scale=1.0):
    """float32 [3][h][w]: the rule's planes of the storage image `logical` [h][w][3]."""
    return np.ascontiguousarray(rule(logical, dtype, scale)[0].transpose(2, 0, 1))


def image_of_planes(planes, dtype, scale=1.0):
    """Storage [h][w][3] of `dtype` holding planes / scale (rounded to the type): what a caller with such data has."""
    v = np.ascontiguousarray(np.asarray(planes, np.float32).transpose(1, 2, 0))
    return to_storage(v / np.float32(scale) if scale != 1.0 else v, dtype)


def pixels_of(mem, src, stream=0):
    """(capi.GzDevicePixels, what keeps the memory alive) of a device_input_cases Source."""
    held = mem.put(src.storage)
    return device_pixels(mem.address(held) + src.offset * src.itemsize, bpc.PIXEL_CODES[src.dtype], src.strides, stream), held


_expected = {}


def expected(chk, lin0, lin1):
    """(distance as the float the library returns, float32 map) of the checker for two images' planes; computed once per
    checker and pair, and handed out read-only."""
    key = (chk.name, lin0.shape, lin0.tobytes(), lin1.tobytes())
    if key not in _expected:
        d, s = chk.diffmap(np.ascontiguousarray(lin0, np.float32), np.ascontiguousarray(lin1, np.float32))
        d.setflags(write=False)
        _expected[key] = (np.float32(s), d)
    return _expected[key]


def linear_context(L, mem, src, scale=1.0):
    px, held = pixels_of(mem, src)
    ctx = L.context_from_device_linear(px, src.w, src.h, scale)
    ctx._held = held
    return ctx


def compare_linear(ctx, mem, src, scale=1.0, dtype="float32", layout="crop", heat=None):
    """gz_compare_device_linear of a Source with a map destination -> (distance, float32 map, clamped); the
    destination's surroundings are checked too.  heat = (good, bad): a uint8 heat map too, appended."""
    px, held = pixels_of(mem, src)
    dest = bpc.map_destination(src.w, src.h, dtype, layout)
    dm, handle = dest.on(mem)
    extra = ()
    if heat:
        hdest = doc.destination(src.w, src.h, "uint8", "HWC_crop")
        hout, hhandle, _ = hc.on_device(mem, hdest)
        d, clamped = ctx.compare_device_linear(px, scale, dm, hout, heat[0], heat[1])
        extra = (hdest, mem.get(hhandle))
    else:
        d, clamped = ctx.compare_device_linear(px, scale, dm)
    raw = mem.get(handle)
    got = np.ascontiguousarray(bpc.widen_map(dest.image_of(raw), dtype))
    dest.check(got, raw, what="around the map", nan_is_nan=True)
    del held
    return (np.float32(d), got, clamped) + extra


# ------------------------------------------------------------------ 1. parity ----
def noise_pair(w, h):
    """Two float32 [3][h][w] images on noise that differ by 0.3 EVERYWHERE: less than a byte step of the sRGB table at
    most levels, so the 8-bit path (which rounds every element to a byte first) cannot see most of it."""
    rng = np.random.default_rng(fields.SEED + w * 131 + h)
    a = (rng.random((3, h, w), dtype=np.float32) * np.float32(254)).astype(np.float32)
    return a, (a + np.float32(0.3)).astype(np.float32)


def parity_pairs(w, h):
    """(name, planes0, planes1): tests/fields.py pairs -- linear [0, 255] fields, off the sRGB table's values -- and the
    0.3 pair."""
    for name, _, lin0, lin1 in fields.pairs(w, h, only=("noise", "primaries")):
        if name.split("/")[1] in ("off_table", "jpeg_error_x3", "inverse"):
            yield name, lin0, lin1
    a, b = noise_pair(w, h)
    yield "noise+0.3", a, b


def check_parity(L, mem, chk, lin0, lin1, what):
    ed, em = expected(chk, lin0, lin1)
    _, h, w = lin0.shape
    with linear_context(L, mem, dic.lay_out(image_of_planes(lin0, "float32"), "float32", "CHW")) as ctx:
        d, m, clamped = compare_linear(ctx, mem, dic.lay_out(image_of_planes(lin1, "float32"), "float32", "HWC"))
        assert_bits_equal(m, em, f"map of {what} {w}x{h}")
        assert bits(d) == bits(ed), (what, d, ed)
        assert clamped == 0


def case_parity(L, mem, chk):
    for w, h in PARITY_SIZES:
        for name, lin0, lin1 in parity_pairs(w, h):
            check_parity(L, mem, chk, lin0, lin1, name)
            check_parity(L, mem, chk, lin1, lin0, name + " swapped")     # the metric is not symmetric
        a, b = noise_pair(w, h)
        assert expected(chk, a, b)[0] > 0 and expected(chk, b, a)[0] > 0
        if (w, h) == (33, 17):
            assert not np.array_equal(expected(chk, a, b)[1], expected(chk, b, a)[1])


def case_the_byte_path_cannot_see_it(L, mem, chk):
    """The same 0.3 pair at levels where 0.3 is under half a step of the byte scale: as [0, 1] float images through the
    8-bit entry both round to the same bytes and compare as distance 0; the linear entry returns the checker's distance,
    which is above 0."""
    w, h = 33, 17
    rng = np.random.default_rng(fields.SEED)
    k = rng.integers(1, 254, (h, w, 3)).astype(np.float32)
    a8, b8 = k / np.float32(255), (k + np.float32(0.3)) / np.float32(255)
    assert np.array_equal(dic.expected_bytes(a8, "float32"), dic.expected_bytes(b8, "float32"))
    rgb = dic.expected_bytes(a8, "float32")
    with L.context(rgb, TARGET) as ctx:
        px, held = bpc.pixels_of(mem, dic.lay_out(b8, "float32", "HWC"))
        assert ctx.compare_device_pixels(px) == 0.0
    lin0, lin1 = planes_of(a8, "float32", 255.0), planes_of(b8, "float32", 255.0)
    ed, em = expected(chk, lin0, lin1)
    assert ed > 0
    with linear_context(L, mem, dic.lay_out(a8, "float32", "HWC"), 255.0) as ctx:
        d, m, _ = compare_linear(ctx, mem, dic.lay_out(b8, "float32", "HWC"), 255.0)
        assert bits(d) == bits(ed) and d > 0
        assert_bits_equal(m, em, "map of the 0.3 pair")


# ------------------------------------------------------------------ 2. every way in ----
def read_path(src):
    """ingest_wide_mode restated: the instantiation of k_ingest_linear the launch code picks for a Source at a 64-byte
    aligned buffer."""
    sy, sx, sc = src.strides
    p = 16 // src.itemsize
    if (src.offset * src.itemsize) % 16 or sy % p:
        return "elementwise"
    if sx == 1 and sc % p == 0:
        return "planar"
    if sc == 1 and sx == 3:
        return "interleaved"
    return "elementwise"


def case_every_way_in(L, mem, chk, dtype):
    """Every layout x width x scale of `dtype`: the planes are the rule's (as the original's and as the other image's),
    the map is the checker's of those planes.  -> the read paths taken."""
    paths = set()
    h = 9
    for w in WIDTHS[dtype]:
        rng = np.random.default_rng(w * 7 + len(dtype))
        base = (rng.random((h, w, 3), dtype=np.float32) * np.float32(255)).astype(np.float32)
        other = np.clip(base + rng.normal(0, 4, base.shape).astype(np.float32), 0, 255).astype(np.float32)
        for scale in (1.0, 255.0):
            # (for scale = 255 the elements are in [0, 1]: x * 255 in float32 stays at or under 255)
            s0 = to_storage(base / np.float32(scale), dtype)
            s1 = to_storage(other / np.float32(scale), dtype)
            for layout in LAYOUTS:
                src0, src1 = dic.lay_out(s0, dtype, layout), dic.lay_out(s1, dtype, layout)
                paths.add(read_path(src0))
                lin0, lin1 = planes_of(src0.logical, dtype, scale), planes_of(src1.logical, dtype, scale)
                assert rule(src0.logical, dtype, scale)[1] == 0 and rule(src1.logical, dtype, scale)[1] == 0
                ed, em = expected(chk, lin0, lin1)
                with linear_context(L, mem, src0, scale) as ctx:
                    assert_bits_equal(ctx.probe_linear_planes(), lin0, f"planes of the original, {dtype} {layout} {w} x{scale}")
                    d, m, clamped = compare_linear(ctx, mem, src1, scale, layout=("contiguous", "crop", "base1")[w % 3])
                    assert_bits_equal(ctx.probe_linear_planes(), lin1, f"planes of the other image, {dtype} {layout} {w} x{scale}")
                    assert_bits_equal(m, em, f"map, {dtype} {layout} {w} x{scale}")
                    assert bits(d) == bits(ed) and clamped == 0
    return paths


# ------------------------------------------------------------------ 3. clamp and count ----
SPECIALS = (np.nan, -1.0, -0.0, 255.5, np.inf, -np.inf)
ALTERED = 5   # of SPECIALS: all but -0.0, which is not below 0


def special_image(w, h, dtype, seed=3):
    """Storage [h][w][3]: values in [0, 255] with every special at known positions -- one set in the first group of a
    row, one in a partial group at a row's end, one per channel."""
    rng = np.random.default_rng(seed)
    v = (rng.random((h, w, 3), dtype=np.float32) * np.float32(255)).astype(np.float32)
    where = []
    for i, s in enumerate(SPECIALS):
        for (y, x, c) in ((1 + i % (h - 1), i % 3, i % 3), (h - 1 - i % 2, w - 1 - i % 2, (i + 1) % 3), (i % h, (5 + 2 * i) % w, (i + 2) % 3)):
            if (y, x, c) not in where:
                v[y, x, c] = s
                where.append((y, x, c))
    st = to_storage(v, dtype)
    return st, rule(st, dtype)[1]


def case_clamp_and_count(L, mem, chk):
    w, h = 17, 9
    for dtype in DTYPES:
        s0, n0 = special_image(w, h, dtype, seed=3)
        s1, n1 = special_image(w, h, dtype, seed=4)
        assert n0 >= 2 * ALTERED and n1 >= 2 * ALTERED
        lin0, lin1 = planes_of(s0, dtype), planes_of(s1, dtype)
        assert np.isfinite(lin0).all() and lin0.min() >= 0 and lin0.max() <= 255
        assert (bits(lin0) == bits(np.float32(-0.0))).any()         # -0.0 stays what it is
        ed, em = expected(chk, lin0, lin1)
        for layout in ("HWC", "CHW", "HWC_crop_base1"):
            with linear_context(L, mem, dic.lay_out(s0, dtype, layout)) as ctx:
                assert_bits_equal(ctx.probe_linear_planes(), lin0, f"clamped planes, {dtype} {layout}")
                d, m, clamped = compare_linear(ctx, mem, dic.lay_out(s1, dtype, layout))
                assert clamped == n1, (dtype, layout, clamped, n1)
                assert_bits_equal(ctx.probe_linear_planes(), lin1, f"clamped planes of the other image, {dtype} {layout}")
                assert_bits_equal(m, em, f"map of the clamped images, {dtype} {layout}")
                assert bits(d) == bits(ed)
            # gz_butteraugli_linear counts both images
            p0, k0 = pixels_of(mem, dic.lay_out(s0, dtype, layout))
            p1, k1 = pixels_of(mem, dic.lay_out(s1, dtype, layout))
            d, clamped = L.butteraugli_linear(p0, p1, w, h)
            assert bits(np.float32(d)) == bits(ed) and clamped == n0 + n1, (dtype, layout, clamped, n0, n1)
    # a scale that pushes ordinary values over the top
    s, n = special_image(w, h, "float32", seed=5)
    lin, n2 = rule(s, "float32", 2.0)
    assert n2 > n
    with linear_context(L, mem, dic.lay_out(s, "float32", "HWC"), 2.0) as ctx:
        assert_bits_equal(ctx.probe_linear_planes(), np.ascontiguousarray(lin.transpose(2, 0, 1)), "scale 2")


# ------------------------------------------------------------------ 4. small images ----
def extended(planes):
    """ButteraugliDiffmap's rule (butteraugli.cc:1825-1845) -> (the 8-canvas planes, xborder, yborder)."""
    _, h, w = planes.shape
    xb, yb = ((8 - w) // 2 if w < 8 else 0), ((8 - h) // 2 if h < 8 else 0)
    xs = np.clip(np.arange(max(w, 8)) - xb, 0, w - 1)
    ys = np.clip(np.arange(max(h, 8)) - yb, 0, h - 1)
    return np.ascontiguousarray(planes[:, ys][:, :, xs]), xb, yb


def expected_small(chk, lin0, lin1):
    """:1846-1855 and ButteraugliScoreFromDiffmap: the checker's map of the two canvases, cropped, and its maximum."""
    _, h, w = lin0.shape
    c0, xb, yb = extended(lin0)
    c1, _, _ = extended(lin1)
    _, full = expected(chk, c0, c1)
    crop = np.ascontiguousarray(full[yb:yb + h, xb:xb + w])
    return np.float32(crop.max()), crop


def case_small_images(L, mem, chk, good, bad):
    for n, (w, h) in enumerate(SMALL_SIZES):
        for dtype in ("float32", "bfloat16"):
            rng = np.random.default_rng(100 * w + h)
            s0 = to_storage(rng.random((h, w, 3), dtype=np.float32) * np.float32(255), dtype)
            s1 = to_storage(np.clip(dic.widen(s0, dtype) + rng.normal(0, 9, (h, w, 3)).astype(np.float32), 0, 255), dtype)
            lin0, lin1 = planes_of(s0, dtype), planes_of(s1, dtype)
            ed, em = expected_small(chk, lin0, lin1)
            if w < 8 and h < 8 and w * h > 1:
                full = expected(chk, extended(lin0)[0], extended(lin1)[0])[1]
                assert full.shape == (8, 8)
            layout = ("HWC", "CHW", "HWC_crop_base1")[n % 3]
            p0, k0 = pixels_of(mem, dic.lay_out(s0, dtype, layout))
            p1, k1 = pixels_of(mem, dic.lay_out(s1, dtype, layout))
            # the destinations: sentinel-filled canvases larger than the image
            mdest = bpc.map_destination(w, h, "float32", "crop")
            dm, mh = mdest.on(mem)
            hdest = doc.destination(w, h, "uint8", "HWC_crop")
            hout, hh, _ = hc.on_device(mem, hdest)
            d, clamped = L.butteraugli_linear(p0, p1, w, h, 1.0, dm, hout, good, bad)
            assert bits(np.float32(d)) == bits(ed), (w, h, dtype, d, ed)
            assert clamped == 0
            mdest.check(em, mem.get(mh), what=f"map of {w}x{h} {dtype}")
            hdest.check(hc.expected_heat(em, good, bad), mem.get(hh), what=f"heat map of {w}x{h} {dtype}")
            # without destinations: the same distance
            assert bits(np.float32(L.butteraugli_linear(p0, p1, w, h)[0])) == bits(ed)
    # a clamped element in a replicated border counts once
    w, h = 3, 5
    s = np.full((h, w, 3), 100, np.float32)
    s[0, 0, 1] = -5
    p, k = pixels_of(mem, dic.lay_out(s, "float32", "HWC"))
    assert L.butteraugli_linear(p, p, w, h)[1] == 2


# ------------------------------------------------------------------ 5. state ----
def state_expecting(call, why):
    try:
        call()
    except GuetzliAmdError as e:
        assert "GZ_E_STATE" in str(e) and why in str(e), str(e)
        return True
    return False


def case_state(L, mem, chk):
    w, h = 33, 17
    a, b = noise_pair(w, h)
    rgb0, rgb1 = bpc.pair("photo", w, h)
    src_a = dic.lay_out(image_of_planes(a, "float32"), "float32", "HWC")
    src_b = dic.lay_out(image_of_planes(b, "float32"), "float32", "CHW")
    with linear_context(L, mem, src_a) as ctx:
        # the entries that need 8-bit pixels or coefficients of the original say why they refuse
        assert state_expecting(lambda: ctx.encode_rgb(), "linear float image")
        assert state_expecting(lambda: ctx.block_zeroing_orders(), "linear float image")
        assert state_expecting(lambda: ctx.quantize(), "linear float image")
        assert state_expecting(lambda: ctx.downsample(), "linear float image")
        # an 8-bit image against the linear original: the checker on (linear original, table-linearised bytes)
        ed, em = expected(chk, a, fields.linear(rgb1))
        d, m = bpc.compare_pixels(ctx, mem, dic.lay_out(rgb1, "uint8", "HWC"), w, h)
        assert_bits_equal(m, em, "8-bit image against a linear original")
        assert bits(d) == bits(ed)
        d2, m2 = ctx.compare_rgb(rgb1)
        assert_bits_equal(m2, em, "compare_rgb against a linear original")
        # ... and the linear one still compares
        ed, em = expected(chk, a, b)
        d, m, _ = compare_linear(ctx, mem, src_b)
        assert_bits_equal(m, em, "linear pair after an 8-bit one")
        # gz_set_rgb: the context equals a fresh 8-bit one
        ctx.set_rgb(rgb0)
        with L.context(rgb0, 1.0) as fresh:      # (a context made for a linear original has the target 1)
            assert np.array_equal(ctx.encode_rgb(), fresh.encode_rgb())
            q = np.full((3, 64), 4, np.int32)
            ctx.quantize(q, download=False)
            fresh.quantize(q, download=False)
            for g, e, name in zip(ctx.compare(), fresh.compare(), ("distance", "distance map", "block maxima")):
                assert_bits_equal(np.asarray(g, np.float32), np.asarray(e, np.float32), f"{name} after gz_set_rgb")
            assert np.array_equal(ctx.block_zeroing_orders()[0], fresh.block_zeroing_orders()[0])
        # a linear image against the 8-bit original (every context takes gz_compare_device_linear)
        ed, em = expected(chk, fields.linear(rgb0), b)
        d, m, _ = compare_linear(ctx, mem, src_b)
        assert_bits_equal(m, em, "linear image against an 8-bit original")
        assert bits(d) == bits(ed)
        # gz_set_linear_device on that context: linear again
        pa, ka = pixels_of(mem, src_a)
        ctx.set_linear_device(pa)
        assert state_expecting(lambda: ctx.encode_rgb(), "linear float image")
        ed, em = expected(chk, a, b)
        d, m, _ = compare_linear(ctx, mem, src_b)
        assert_bits_equal(m, em, "after gz_set_linear_device")
        assert bits(d) == bits(ed)


def case_pending_compare_refuses(L, mem):
    w, h = 33, 17
    rgb0, _ = bpc.pair("photo", w, h)
    a, b = noise_pair(w, h)
    src = dic.lay_out(image_of_planes(b, "float32"), "float32", "HWC")
    px, held = pixels_of(mem, src)
    with L.context(rgb0, TARGET) as ctx:
        ctx.encode_rgb(download=False)
        ctx.quantize(bpc.Q, download=False)
        exp = ctx.compare()
        ctx.compare_begin()
        assert state_expecting(lambda: ctx.compare_device_linear(px), "in flight")
        assert state_expecting(lambda: ctx.set_linear_device(px), "in flight")
        assert bits(np.float32(ctx.compare_end())) == bits(np.float32(exp[0]))
        assert bits(np.float32(ctx.compare_device_linear(px)[0])) == bits(expected(oracle, fields.linear(rgb0), b)[0])
