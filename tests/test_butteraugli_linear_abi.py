"""CPU: what the linear float entries of the PRODUCT library (gz_create_from_device_linear / gz_set_linear_device /
gz_compare_device_linear / gz_butteraugli_linear) refuse from their arguments alone, before any device call -- so the
answers are the same with and without a GPU -- and, without one, that valid arguments ask for the device and fail
loudly with GZ_E_NO_DEVICE."""
import ctypes as C

import numpy as np
import pytest

from guetzli_amd import build as gzbuild
from guetzli_amd import capi
from guetzli_amd.capi import device_map, device_output, device_pixels

W, H = 33, 17
GOOD, BAD = 0.6, 1.7


@pytest.fixture(scope="module")
def lib():
    return capi.Library(gzbuild.build()).lib


def images():
    a = np.zeros((H, W, 3), np.float32)
    return a, device_pixels(a.ctypes.data, capi.GZ_DT_F32, (3 * W, 3, 1))


def bad_images(ptr):
    def p(**kw):
        a = dict(dict(ptr=ptr, dtype=capi.GZ_DT_F32, strides=(3 * W, 3, 1), alpha=0), **kw)
        return device_pixels(a["ptr"], a["dtype"], a["strides"], 0, a["alpha"])
    wrong_size = p()
    wrong_size.struct_size -= 8
    return [p(dtype=capi.GZ_DT_U8), p(dtype=capi.GZ_DT_U16), p(dtype=-1), p(dtype=5),      # integers, and no dtype at all
            p(alpha=ptr + 12), p(dtype=capi.GZ_DT_F16, alpha=ptr),                         # alpha set
            p(ptr=0), wrong_size, p(strides=(-3 * W, 3, 1)), p(strides=(3 * W, 3, -1)), p(strides=(1 << 59, 3, 1))]


BAD_SCALES = (0.0, -1.0, -0.0, float("nan"), float("inf"), float("-inf"))


def bad_maps(ptr):
    def m(**kw):
        a = dict(dict(ptr=ptr, dtype=capi.GZ_DT_F32, strides=(W, 1)), **kw)
        return device_map(a["ptr"], a["dtype"], a["strides"])
    return [m(strides=(0, 1)), m(strides=(W, 0)), m(strides=(1, 1)), m(strides=(W - 1, 1)), m(strides=(1, H - 1)),   # aliasing
            m(strides=(-W, 1)), m(dtype=capi.GZ_DT_U8), m(ptr=0)]


def test_refusals_without_a_device(lib):
    a, good = images()
    out = np.zeros((H, W), np.float32)
    heat = np.zeros((H, W, 3), np.uint8)
    dist = np.zeros(1, np.float32)
    clamped = C.c_uint64(7)
    good_map = device_map(out.ctypes.data, capi.GZ_DT_F32, (W, 1))
    good_heat = device_output(heat.ctypes.data, capi.GZ_DT_U8, (3 * W, 3, 1))
    err = C.c_int(0)

    def create(px, scale, w=W, h=H):
        err.value = 0
        assert not lib.gz_create_from_device_linear(0, w, h, None if px is None else C.byref(px), scale, C.byref(err))
        return err.value

    def whole(p0, p1, scale, dm=None, ho=None, good_=GOOD, bad_=BAD, w=W, h=H, d=dist):
        return lib.gz_butteraugli_linear(0, w, h, None if p0 is None else C.byref(p0), None if p1 is None else C.byref(p1), scale,
                                         None if d is None else d.ctypes.data, None if dm is None else C.byref(dm),
                                         None if ho is None else C.byref(ho), good_, bad_, C.byref(clamped))

    for px in bad_images(a.ctypes.data):
        assert create(px, 1.0) == -1
        assert whole(px, good, 1.0) == -1 and whole(good, px, 1.0) == -1
    for scale in BAD_SCALES:
        assert create(good, scale) == -1
        assert whole(good, good, scale) == -1
    for dm in bad_maps(out.ctypes.data):
        assert whole(good, good, 1.0, dm) == -1
    assert create(None, 1.0) == -1 and whole(None, good, 1.0) == -1 and whole(good, None, 1.0) == -1
    assert whole(good, good, 1.0, d=None) == -1
    # a context is 8 x 8 at the least; ButteraugliInterface takes every size from 1 x 1, but none below
    for w, h in ((7, H), (W, 7), (0, H), (W, 1 << 16)):
        assert create(good, 1.0, w, h) == -1
    for w, h in ((0, H), (W, 0), (-1, H), (1 << 16, H)):
        assert whole(good, good, 1.0, w=w, h=h) == -1
    # the heat map's thresholds and its destination, as for the 8-bit entry
    for g, b in ((0.0, 1.0), (1.0, 1.0), (2.0, 1.0), (1.0, float("inf")), (float("nan"), 1.0)):
        assert whole(good, good, 1.0, None, good_heat, g, b) == -1
    aliasing = device_output(heat.ctypes.data, capi.GZ_DT_U8, (3 * W, 3, 0))
    assert whole(good, good, 1.0, None, aliasing) == -1
    # the context entries: no context, no call
    assert lib.gz_set_linear_device(None, C.byref(good), 1.0) == -1
    assert lib.gz_compare_device_linear(None, C.byref(good), 1.0, dist.ctypes.data, None, None, GOOD, BAD, None) == -1
    assert lib.gz_probe_linear_planes(None, out.ctypes.data) == -1
    assert dist[0] == 0 and clamped.value == 7 and not out.any() and not heat.any()
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:   # valid arguments: the device is asked for, and there is none -- no fallback
        assert create(good, 1.0) == -2
        assert whole(good, good, 255.0, good_map, good_heat) == -2
        assert whole(good, good, 1.0, w=1, h=1) == -2


def test_refusals_on_a_context_come_before_any_device_call():
    """The same through the CPU emulation, where a context exists: gz_set_linear_device and gz_compare_device_linear
    refuse the bad images, scales and maps without a launch, an allocation or an enqueue."""
    import os
    import sys
    sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")]
    import build_emu
    L = capi.Library(build_emu.build())
    lib = L.lib
    lib.gz_emu_alloc_calls.restype = C.c_long
    lib.gz_emu_launch_calls.restype = C.c_long
    lib.gz_emu_enqueue_log_fetch.restype = C.c_long
    lib.gz_emu_enqueue_log_fetch.argtypes = [C.c_char_p, C.c_long]
    a, good = images()
    a[...] = 100
    out = np.zeros((H, W), np.float32)
    dist = np.zeros(1, np.float32)
    good_map = device_map(out.ctypes.data, capi.GZ_DT_F32, (W, 1))
    with L.context_from_device_linear(good, W, H) as ctx:
        launches, allocs = lib.gz_emu_launch_calls(), lib.gz_emu_alloc_calls()
        lib.gz_emu_enqueue_log_start()
        for px in bad_images(a.ctypes.data):
            assert lib.gz_set_linear_device(ctx.handle, C.byref(px), 1.0) == -1
            assert lib.gz_compare_device_linear(ctx.handle, C.byref(px), 1.0, dist.ctypes.data, C.byref(good_map), None, GOOD, BAD, None) == -1
        for scale in BAD_SCALES:
            assert lib.gz_set_linear_device(ctx.handle, C.byref(good), scale) == -1
            assert lib.gz_compare_device_linear(ctx.handle, C.byref(good), scale, dist.ctypes.data, None, None, GOOD, BAD, None) == -1
        for dm in bad_maps(out.ctypes.data):
            assert lib.gz_compare_device_linear(ctx.handle, C.byref(good), 1.0, dist.ctypes.data, C.byref(dm), None, GOOD, BAD, None) == -1
        assert lib.gz_compare_device_linear(ctx.handle, None, 1.0, dist.ctypes.data, None, None, GOOD, BAD, None) == -1
        assert lib.gz_compare_device_linear(ctx.handle, C.byref(good), 1.0, None, None, None, GOOD, BAD, None) == -1
        lib.gz_emu_enqueue_log_stop()
        assert lib.gz_emu_enqueue_log_fetch(None, 0) == 0             # no copy, no event, no synchronise either
        assert (lib.gz_emu_launch_calls(), lib.gz_emu_alloc_calls()) == (launches, allocs)
        assert not out.any() and dist[0] == 0
        # ... and the context is as it was: the image against itself
        d, clamped = ctx.compare_device_linear(good, 1.0, good_map)
        assert d == 0.0 and clamped == 0 and not out.any()
