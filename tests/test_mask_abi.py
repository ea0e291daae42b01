"""CPU: what the masking entries of the PRODUCT library (gz_opsin_device / gz_mask_device / gz_adaptive_quantization)
refuse from their arguments alone, before any device call -- so the answers are the same with and without a GPU -- and,
without one, that valid arguments ask for the device and fail loudly with GZ_E_NO_DEVICE."""
import ctypes as C

import numpy as np
import pytest

from guetzli_amd import build as gzbuild
from guetzli_amd import capi
from guetzli_amd.capi import GZ_SAMPLES_LINEAR, GZ_SAMPLES_SRGB8, device_map, device_output, device_pixels

W, H = 33, 17
E_ARG, E_NO_DEVICE = -1, -2


@pytest.fixture(scope="module")
def lib():
    return capi.Library(gzbuild.build()).lib


def test_refusals_without_a_device(lib):
    a = np.zeros((H, W, 3), np.float32)
    bytes_ = np.zeros((H, W, 3), np.uint8)
    out, out_dc = np.zeros((3, H, W), np.float32), np.zeros((3, H, W), np.float32)
    plane = np.zeros((H, W), np.float32)
    clamped = C.c_uint64(7)
    lin = device_pixels(a.ctypes.data, capi.GZ_DT_F32, (3 * W, 3, 1))
    u8 = device_pixels(bytes_.ctypes.data, capi.GZ_DT_U8, (3 * W, 3, 1))
    chw = (W, 1, W * H)
    good = device_output(out.ctypes.data, capi.GZ_DT_F32, chw)
    good_dc = device_output(out_dc.ctypes.data, capi.GZ_DT_BF16, chw)
    good_map = device_map(plane.ctypes.data, capi.GZ_DT_F32, (W, 1))
    ref = lambda x: None if x is None else C.byref(x)

    def opsin(img, xyb, samples=GZ_SAMPLES_LINEAR, scale=1.0, w=W, h=H):
        return lib.gz_opsin_device(0, w, h, ref(img), samples, scale, ref(xyb), C.byref(clamped))

    def mask(img0, img1, m, dc, samples=GZ_SAMPLES_LINEAR, scale=1.0, w=W, h=H):
        return lib.gz_mask_device(0, w, h, ref(img0), ref(img1), samples, scale, ref(m), ref(dc), C.byref(clamped))

    def quant(img, q, scale=1.0, w=W, h=H):
        return lib.gz_adaptive_quantization(0, w, h, ref(img), scale, ref(q), C.byref(clamped))

    # sizes: the reference's 16 for the quantisation field, a context's 8 for the other two
    assert quant(lin, good_map, w=15, h=16) == E_ARG and quant(lin, good_map, w=16, h=15) == E_ARG
    assert mask(lin, None, good, None, w=7, h=9) == E_ARG and opsin(lin, good, w=7, h=9) == E_ARG
    assert mask(lin, None, good, None, w=9, h=7) == E_ARG and opsin(lin, good, w=9, h=7) == E_ARG
    for w, h in ((0, H), (W, 0), (-1, H), (1 << 16, H)):
        assert quant(lin, good_map, w=w, h=h) == E_ARG and mask(lin, None, good, None, w=w, h=h) == E_ARG and opsin(lin, good, w=w, h=h) == E_ARG
    # outputs: an integer element type, none at all, strides under which elements share an address
    for dtype in (capi.GZ_DT_U8, capi.GZ_DT_U16, -1, 5):
        bad = device_output(out.ctypes.data, dtype, chw)
        assert opsin(lin, bad) == E_ARG and mask(lin, None, bad, None) == E_ARG and mask(lin, None, None, bad) == E_ARG
        assert mask(lin, None, good, bad) == E_ARG
    assert quant(lin, device_map(plane.ctypes.data, capi.GZ_DT_U8, (W, 1))) == E_ARG
    assert mask(lin, None, None, None) == E_ARG and mask(lin, lin, None, None) == E_ARG
    assert opsin(lin, None) == E_ARG and quant(lin, None) == E_ARG
    for strides in ((W, 1, 0), (W, 1, W), (0, 1, W * H), (W - 1, 1, W * H), (-W, 1, W * H)):
        bad = device_output(out.ctypes.data, capi.GZ_DT_F32, strides)
        assert opsin(lin, bad) == E_ARG and mask(lin, None, bad, None) == E_ARG and mask(lin, lin, good, bad) == E_ARG
    for strides in ((0, 1), (W, 0), (W - 1, 1), (-W, 1)):
        assert quant(lin, device_map(plane.ctypes.data, capi.GZ_DT_F32, strides)) == E_ARG
    assert opsin(lin, device_output(0, capi.GZ_DT_F32, chw)) == E_ARG
    # samples: 0 and 1 are all there is; integers are no linear samples
    for samples in (2, -1):
        assert opsin(lin, good, samples) == E_ARG and mask(lin, None, good, None, samples) == E_ARG
    assert opsin(u8, good, GZ_SAMPLES_LINEAR) == E_ARG and mask(u8, None, good, None, GZ_SAMPLES_LINEAR) == E_ARG
    assert mask(lin, u8, good, None, GZ_SAMPLES_LINEAR) == E_ARG and quant(u8, good_map) == E_ARG
    # images: none, alpha on a linear one, a scale that is no finite positive float
    assert opsin(None, good) == E_ARG and mask(None, lin, good, None) == E_ARG and quant(None, good_map) == E_ARG
    with_alpha = device_pixels(a.ctypes.data, capi.GZ_DT_F32, (3 * W, 3, 1), 0, a.ctypes.data)
    assert opsin(with_alpha, good) == E_ARG and mask(lin, with_alpha, good, None) == E_ARG and quant(with_alpha, good_map) == E_ARG
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        assert opsin(lin, good, scale=scale) == E_ARG and mask(lin, None, good, None, scale=scale) == E_ARG and quant(lin, good_map, scale) == E_ARG
    assert clamped.value == 7 and not out.any() and not out_dc.any() and not plane.any()
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:   # valid arguments: the device is asked for, and there is none -- no fallback
        assert opsin(lin, good) == E_NO_DEVICE and opsin(u8, good, GZ_SAMPLES_SRGB8, scale=0.0) == E_NO_DEVICE
        assert mask(lin, lin, good, good_dc) == E_NO_DEVICE and mask(u8, None, None, good_dc, GZ_SAMPLES_SRGB8) == E_NO_DEVICE
        assert quant(lin, good_map, 255.0, w=16, h=16) == E_NO_DEVICE


def test_the_abi_version_stays():
    """The entries were ADDED: no existing declaration changed, so the version is what it was."""
    assert capi.Library(gzbuild.build()).lib.gz_abi_version() == 6
