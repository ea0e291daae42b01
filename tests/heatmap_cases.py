"""Shared by tests/test_heatmap_emu.py (CPU emulation: "device memory" is host memory), tests/test_heatmap_gpu.py
(memory of the MI355X) and tests/test_heatmap_reference.py: butteraugli's heat map of a distance map --
gz_probe_emit_heat, gz_heatmap_from_map_device, gz_heatmap_device, gz_compare_device_pixels_heat.

What judges the results: score_to_rgb below, a plain-Python restatement of ScoreToRgb (butteraugli.cc:1938-1975) with
math.pow, and of ButteraugliFuzzyClass / ButteraugliFuzzyInverse (:1903-1934) with math.exp.  CPython's math.pow and
math.exp call the process's libm, as the library's threshold table and fuzzy functions do, so both sides agree on any
machine; tests/test_heatmap_reference.py pins the restatement to the reference itself where that is built.  Every
comparison is for equality.

A case takes `mem`, which says where device memory is (butteraugli_pair_cases.HostMemory, or the GPU suite's)."""
import ctypes as C
import math
import os

import numpy as np

import butteraugli_pair_cases as bpc
import device_input_cases as dic
import device_output_cases as doc
from guetzli_amd.capi import GuetzliAmdError, device_output

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heatmap")
DTYPES = doc.DTYPES
CODES = {"uint8": 0, "float32": 1, "float16": 2, "bfloat16": 3, "uint16": 4}
# HWC / CHW contiguous, crops inside a sentinel canvas, the base off by one element, a row pitch that is no multiple of
# 16 bytes, x outermost (device_output_cases.destination)
LAYOUTS = doc.LAYOUTS
WIDTHS = (1, 3, 4, 5, 15, 16, 17, 33, 67)
HEIGHTS = (1, 2, 9)
SIZES = tuple((w, h) for h in HEIGHTS for w in WIDTHS)
PLANE_W, PLANE_H = 67, 17                # the largest plane any synthetic case uses
PHOTO_SIZES = ((64, 17), (67, 9))
OTHER_THRESHOLDS = (0.5, 2.25)           # a second, non-default pair (good, bad)

HEATMAP = ((0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0), (1, 1, 0), (1, 0, 0), (1, 0, 1), (0.5, 0.5, 1.0), (1.0, 0.5, 0.5),
           (1.0, 1.0, 0.5), (1, 1, 1), (1, 1, 1))


# ------------------------------------------------------------------ the restatement ----
def fuzzy_class(score):
    fuzzy_width_up = 6.07887388532
    fuzzy_width_down = 5.50793514384
    m0 = 2.0
    scaler = 0.840253347958
    if score < 1.0:
        val = m0 / (1.0 + math.exp((score - 1.0) * fuzzy_width_down))
        val -= 1.0
        val *= 2.0 - scaler
        val += scaler
    else:
        val = m0 / (1.0 + math.exp((score - 1.0) * fuzzy_width_up))
        val *= scaler
    return val


def fuzzy_inverse(seek):
    pos = 0.0
    rng = 1.0
    while rng >= 1e-10:
        if fuzzy_class(pos) < seek:
            pos -= rng
        else:
            pos += rng
        rng *= 0.5
    return pos


def default_thresholds():
    return fuzzy_inverse(1.5), fuzzy_inverse(0.5)


def score_to_rgb(score, good, bad):
    """ScoreToRgb of one distance (a Python float holding the float32's value) -> (r, g, b)."""
    if score < good:
        score = (score / good) * 0.3
    elif score < bad:
        score = 0.3 + (score - good) / (bad - good) * 0.15
    else:
        score = 0.45 + (score - bad) / (bad * 12) * 0.5
    score = score * 11
    score = 0.0 if score < 0.0 else score      # std::max<double>(score * 11, 0.0)
    score = 10.0 if 10.0 < score else score    # std::min<double>(.., 10)
    ix = int(score)
    mix = score - ix
    return tuple(int(255 * math.pow(mix * HEATMAP[ix + 1][c] + (1 - mix) * HEATMAP[ix][c], 0.5) + 0.5) for c in range(3))


_heat = {}


def expected_heat(plane, good, bad):
    """uint8 [h][w][3]: CreateHeatMapImage of the float32 `plane` by the restatement; computed once per plane and pair of
    thresholds, and handed out read-only."""
    p = np.ascontiguousarray(plane, np.float32)
    key = (p.shape, p.tobytes(), good, bad)
    if key not in _heat:
        out = np.array([score_to_rgb(float(d), good, bad) for d in p.ravel()], np.uint8).reshape(p.shape + (3,))
        out.setflags(write=False)
        _heat[key] = out
    return _heat[key]


# ------------------------------------------------------------------ synthetic distances ----
def neighbours(values, reach=2):
    """float32: every value with the `reach` floats to either side of it."""
    v = np.asarray(values, np.float64).astype(np.float32)
    out = [v]
    lo = hi = v
    for _ in range(reach):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return np.stack(out, -1).reshape(-1)


def threshold_distances(good):
    """[255][5]: for k = 1 .. 255 the float nearest ((k - 0.5) / 255)^2 good / 3.3 and two floats to either side.  In the
    first colour segment blue is v = mix = (d / good) 0.3 11: these floats straddle the threshold of every byte."""
    return neighbours([((k - 0.5) / 255) ** 2 * good / 3.3 for k in range(1, 256)]).reshape(255, 5)


def boundary_distances(good, bad):
    """good, bad, and the distances where score * 11 is an integer (a new pair of table rows), with their neighbours."""
    d = [good, bad]
    d += [j / 3.3 * good for j in (1, 2, 3)]
    d += [good + (4 / 11 - 0.3) / 0.15 * (bad - good)]
    d += [bad + (j / 11 - 0.45) * 24 * bad for j in range(5, 12)]
    return neighbours(d)


def special_distances():
    return np.array([0.0, -0.0, -1.0, np.inf, np.finfo(np.float32).max, 1e-45], np.float32)


def sweep_distances(bad):
    return np.linspace(0, 14 * bad, 4096).astype(np.float32)


def segments_of(values, good, bad):
    """The table row ix of every distance (the restatement's own)."""
    rows = set()
    for d in np.asarray(values, np.float32):
        s = float(d)
        s = (s / good) * 0.3 if s < good else 0.3 + (s - good) / (bad - good) * 0.15 if s < bad else 0.45 + (s - bad) / (bad * 12) * 0.5
        rows.add(int(min(max(s * 11, 0.0), 10.0)))
    return rows


def assert_the_cases_reach_what_they_claim(good, bad):
    """(of the restatement, before it judges the library) both bytes k - 1 and k of blue appear among the five floats of
    every k; the sweep visits all 11 segments."""
    t = threshold_distances(good)
    blue = expected_heat(t, good, bad)[:, :, 2]
    for k in range(1, 256):
        assert {k - 1, k} <= set(blue[k - 1].tolist()), (k, blue[k - 1])
    assert segments_of(sweep_distances(bad), good, bad) == set(range(11))


_planes = {}


def synthetic_planes(good, bad):
    """float32 [n][PLANE_H][PLANE_W]: the threshold, sweep, boundary and special distances of (good, bad), the tail
    filled with the sweep again."""
    key = (good, bad)
    if key not in _planes:
        flat = np.concatenate([special_distances(), threshold_distances(good).reshape(-1), boundary_distances(good, bad),
                               sweep_distances(bad)])
        per = PLANE_W * PLANE_H
        n = -(-flat.size // per)
        flat = np.concatenate([flat, sweep_distances(bad)[:n * per - flat.size]])
        p = flat.reshape(n, PLANE_H, PLANE_W)
        p.setflags(write=False)
        _planes[key] = p
    return _planes[key]


def plane_of_size(w, h, good, bad, seed):
    """float32 [h][w] drawn from the synthetic distances of (good, bad): every kind of value at every shape."""
    pool = synthetic_planes(good, bad).reshape(-1)
    return np.ascontiguousarray(pool[np.random.default_rng(seed).integers(0, pool.size, (h, w))])


def golden_plane(good, bad):
    """The plane tools/gen_heatmap_golden.py records the reference's heat map of."""
    return plane_of_size(PLANE_W, PLANE_H, good, bad, seed=20261019)


def golden():
    """(plane float32 [17][67], heat uint8 [17][67][3], good, bad): the reference's own output, recorded by
    tools/gen_heatmap_golden.py."""
    plane = np.load(os.path.join(GOLDEN, "plane_67x17.npy"))
    heat = np.load(os.path.join(GOLDEN, "heat_67x17.npy"))
    assert plane.shape == (17, 67) and plane.dtype == np.float32 and heat.shape == (17, 67, 3) and heat.dtype == np.uint8
    return plane, heat


# ------------------------------------------------------------------ destinations ----
def store_path(address, itemsize, strides):
    """ingest_wide_mode restated: which instantiation of k_emit_heat the launch code picks for a destination."""
    sy, sx, sc = strides
    p = 16 // itemsize
    if address % 16 or sy % p:
        return "elementwise"
    if sx == 1 and sc % p == 0:
        return "planar"
    if sc == 1 and sx == 3:
        return "interleaved"
    return "elementwise"


def on_device(mem, dest, stream=0):
    """(capi.GzDeviceOutput, the handle of the buffer in device memory, the store path it takes)."""
    handle = mem.put(dest.raw)
    address = mem.address(handle) + dest.offset * dest.itemsize
    return device_output(address, CODES[dest.dtype], dest.strides, stream), handle, store_path(address, dest.itemsize, dest.strides)


# ------------------------------------------------------------------ cases ----
def case_probe_values(L, mem, good, bad):
    """Every synthetic distance of (good, bad) through gz_probe_emit_heat, as uint8 HWC and float32 CHW."""
    assert_the_cases_reach_what_they_claim(good, bad)
    for i, plane in enumerate(synthetic_planes(good, bad)):
        for dtype, layout in (("uint8", "HWC"), ("float32", "CHW")):
            dest = doc.destination(PLANE_W, PLANE_H, dtype, layout)
            out, handle, _ = on_device(mem, dest)
            L.probe_emit_heat(plane, good, bad, out)
            dest.check(expected_heat(plane, good, bad), mem.get(handle), what=f"synthetic plane {i}, {good}, {bad}")


def case_golden(L, mem, good, bad):
    plane, heat = golden()
    assert np.array_equal(expected_heat(plane, good, bad), heat)
    dest = doc.destination(PLANE_W, PLANE_H, "uint8", "HWC")
    out, handle, _ = on_device(mem, dest)
    L.probe_emit_heat(plane, good, bad, out)
    dest.check(heat, mem.get(handle), what="the reference's recorded heat map")


def case_probe_shapes(L, mem, dtype, layout, good, bad):
    """gz_probe_emit_heat over every width x height: the restatement's bytes as elements, untouched surroundings.
    -> the store paths taken."""
    paths = set()
    for w, h in SIZES:
        plane = plane_of_size(w, h, good, bad, seed=100 * h + w)
        dest = doc.destination(w, h, dtype, layout)
        out, handle, path = on_device(mem, dest)
        paths.add(path)
        L.probe_emit_heat(plane, good, bad, out)
        dest.check(expected_heat(plane, good, bad), mem.get(handle), what=(layout, w, h))
    return paths


def case_from_map_shapes(L, mem, dtype, layout, good, bad):
    """gz_heatmap_from_map_device on the same planes, in device memory with a pitch of w and of w + 3 floats, the
    plane's base 16-byte aligned and one float further on."""
    paths = set()
    for n, (w, h) in enumerate(SIZES):
        plane = plane_of_size(w, h, good, bad, seed=100 * h + w)
        pitch, lead = w + 3 * (n % 2), (n // 2) % 2
        held = np.full(lead + h * pitch, np.float32(np.nan), np.float32)
        np.lib.stride_tricks.as_strided(held[lead:], (h, w), (4 * pitch, 4))[...] = plane
        src = mem.put(held)
        dest = doc.destination(w, h, dtype, layout)
        out, handle, path = on_device(mem, dest)
        paths.add(path)
        L.heatmap_from_map_device(mem.address(src) + 4 * lead, w, h, pitch, good, bad, out)
        dest.check(expected_heat(plane, good, bad), mem.get(handle), what=(layout, w, h, pitch, lead))
        assert np.array_equal(mem.get(src).view(np.uint32), held.view(np.uint32))
    return paths


def heat_now(ctx, mem, w, h, good, bad, dtype="uint8", layout="HWC_crop"):
    dest = doc.destination(w, h, dtype, layout)
    out, handle, _ = on_device(mem, dest)
    ctx.heatmap_device(good, bad, out)
    return dest, mem.get(handle)


def case_compare_with_heat(L, mem, chk, good, bad):
    """gz_compare_device_pixels_heat with and without a map, and gz_heatmap_device behind it: the restatement applied to
    the checker's distance map."""
    for (w, h), (dtype, layout) in zip(PHOTO_SIZES, (("uint8", "HWC"), ("float16", "CHW_crop"))):
        rgb0, rgb1 = bpc.pair("photo", w, h)
        ed, em = bpc.expected(chk, rgb0, rgb1)
        heat = expected_heat(em, good, bad)
        assert len(np.unique(heat.reshape(-1, 3), axis=0)) > 8        # (a picture, not one colour)
        with L.context(rgb0, bpc.TARGET) as ctx:
            px, held = bpc.pixels_of(mem, dic.lay_out(rgb1, "uint8", "HWC"))
            for with_map in (False, True):
                dest = doc.destination(w, h, dtype, layout)
                out, handle, _ = on_device(mem, dest)
                mdest = bpc.map_destination(w, h, "float32", "crop")
                dm, mhandle = mdest.on(mem)
                d = ctx.compare_device_pixels_heat(px, out, good, bad, dm if with_map else None)
                assert bpc.bits(np.float32(d)) == bpc.bits(ed)
                dest.check(heat, mem.get(handle), what=("compare with heat", w, h, with_map))
                if with_map:
                    mdest.check(em, mem.get(mhandle), what="the map beside the heat map")
                else:
                    assert np.array_equal(mem.get(mhandle), mdest.before)
                for dt2, lay2 in (("uint8", "HWC_crop"), ("bfloat16", "CHW"), ("uint16", "WHC")):   # the map was stored either way
                    d2, raw = heat_now(ctx, mem, w, h, good, bad, dt2, lay2)
                    d2.check(heat, raw, what=("gz_heatmap_device", dt2, lay2))
                other = expected_heat(em, *OTHER_THRESHOLDS)
                d2, raw = heat_now(ctx, mem, w, h, *OTHER_THRESHOLDS)
                d2.check(other, raw, what="other thresholds")
            # with the heat argument NULL it is gz_compare_device_pixels
            dist = np.zeros(1, np.float32)
            assert L.lib.gz_compare_device_pixels_heat(ctx.handle, C.byref(px), dist.ctypes.data, None, None, good, bad) == 0
            assert bpc.bits(dist[0]) == bpc.bits(ed)
            del held


def heat_refused(ctx, mem, w, h, good, bad):
    dest = doc.destination(w, h, "uint8", "HWC")
    out, handle, _ = on_device(mem, dest)
    try:
        ctx.heatmap_device(good, bad, out)
    except GuetzliAmdError as e:
        assert "GZ_E_STATE" in str(e)
        assert np.array_equal(mem.get(handle), dest.before)
        return True
    return False


def case_state(L, mem, good, bad):
    """gz_heatmap_device follows the last stored map: GZ_E_STATE before any comparison, after one that stored none, and
    inside gz_compare_begin .. gz_compare_end; it changes no claim: the next gz_compare is a fresh context's."""
    w, h = 33, 17
    rgb0, rgb1 = bpc.pair("photo", w, h)
    with L.context(rgb0, bpc.TARGET) as fresh:
        fresh.encode_rgb(download=False)
        fresh.quantize(bpc.Q, download=False)
        exp = fresh.compare()
    with L.context(rgb0, bpc.TARGET) as ctx:
        assert heat_refused(ctx, mem, w, h, good, bad)               # nothing compared yet
        ctx.encode_rgb(download=False)
        ctx.quantize(bpc.Q, download=False)
        ctx.compare(want_distmap=False)
        assert heat_refused(ctx, mem, w, h, good, bad)               # the last comparison stored no map
        px, held = bpc.pixels_of(mem, dic.lay_out(rgb1, "uint8", "HWC"))
        ctx.compare_device_pixels(px)
        assert heat_refused(ctx, mem, w, h, good, bad)
        _, dm, _ = ctx.compare()
        dest, raw = heat_now(ctx, mem, w, h, good, bad)
        dest.check(expected_heat(dm, good, bad), raw, what="after gz_compare")
        bpc._assert_compare_equal(ctx.compare(), exp, "gz_compare behind gz_heatmap_device")
        ctx.compare_begin()
        assert heat_refused(ctx, mem, w, h, good, bad)               # a Compare in flight
        ctx.compare_end()
        _, pm = ctx.compare_rgb(rgb1)
        dest, raw = heat_now(ctx, mem, w, h, good, bad, "float32", "CHW_crop_base1")
        dest.check(expected_heat(pm, good, bad), raw, what="after gz_compare_rgb")
        bpc._assert_compare_equal(ctx.compare(), exp, "gz_compare behind a pixel comparison and its heat map")
        del held


# ------------------------------------------------------------------ the reference itself ----
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libgz_ref.so")


def reference_helper(directory):
    """tests/cpp/heatmap_ref.cc compiled into `directory` against oracle/_ref/libgz_ref.so and loaded -> the ctypes
    library (ref_heatmap, ref_fuzzy_class, ref_fuzzy_inverse), or None where the reference is not built."""
    import subprocess
    if not os.path.exists(REF_LIB):
        return None
    so = os.path.join(str(directory), "libheatmap_ref.so")
    subprocess.run(["g++", "-O1", "-std=c++11", "-fPIC", "-shared", os.path.join(ROOT, "tests", "cpp", "heatmap_ref.cc"), "-o", so,
                    "-L" + os.path.dirname(REF_LIB), "-l:libgz_ref.so", "-Wl,-rpath," + os.path.dirname(REF_LIB)], check=True)
    lib = C.CDLL(so)
    lib.ref_heatmap.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p]
    lib.ref_heatmap.restype = None
    for f in (lib.ref_fuzzy_class, lib.ref_fuzzy_inverse):
        f.argtypes, f.restype = [C.c_double], C.c_double
    return lib


def reference_heat(lib, plane, good, bad):
    """uint8 [h][w][3]: butteraugli::CreateHeatMapImage of the float32 `plane`."""
    p = np.ascontiguousarray(plane, np.float32)
    out = np.zeros(p.shape + (3,), np.uint8)
    lib.ref_heatmap(p.ctypes.data, p.shape[1], p.shape[0], good, bad, out.ctypes.data)
    return out
