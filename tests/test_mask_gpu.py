"""Butteraugli's masking on the MI355X: gz_opsin_device / gz_mask_device / gz_adaptive_quantization on memory of torch
tensors -- the cases of tests/mask_cases.py, which tests/test_mask_emu.py runs through the CPU emulation -- and
guetzli_amd.opsin_dynamics / mask / adaptive_quantization on torch tensors.  Here the 16-byte loads and stores and the
FP64 table look-ups are the device's own.  Expectations come from the checkers under oracle/ (the CPU restatement, and
the unmodified reference behind oracle/_ref where it is built); every comparison is bitwise."""
import ctypes as C

import numpy as np
import pytest

import butteraugli_linear_cases as blc
import butteraugli_pair_cases as bpc
import device_input_cases as dic
import mask_cases as mc
from checkers import assert_bits_equal, oracle, ref

pytestmark = pytest.mark.gpu

CHK = ref or oracle


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def L(torch):   # (behind torch: the process then has one HIP runtime, torch's, which the library's NEEDED entry resolves to)
    import guetzli_amd
    return guetzli_amd.load()


@pytest.fixture(scope="module")
def mem(torch):
    class TorchMemory:
        """Device memory: a numpy buffer copied to the GPU (torch's allocations are aligned as the cases assume)."""

        def put(self, array):
            t = torch.from_numpy(np.ascontiguousarray(array)).cuda()
            assert t.data_ptr() % 64 == 0
            return t

        def address(self, handle):
            return handle.data_ptr()

        def get(self, handle):
            return handle.cpu().numpy()
    return TorchMemory()


# ------------------------------------------------------------------ the cases shared with the emulation ----
def test_the_quantisation_field_is_the_references(L, mem):
    mc.case_quant_parity(L, mem, CHK)


def test_mask_of_pairs_in_both_orders_and_of_one_image(L, mem):
    mc.case_mask_parity(L, mem, CHK)


def test_the_opsin_image_is_the_references(L, mem):
    mc.case_opsin_parity(L, mem, CHK)


@pytest.mark.parametrize("dtype", mc.DTYPES)
def test_every_way_out(L, mem, dtype):
    assert mc.case_every_way_out(L, mem, CHK, dtype) == {"wide", "elementwise"}


@pytest.mark.parametrize("dtype", mc.DTYPES)
def test_every_way_in(L, mem, dtype):
    assert mc.case_every_way_in(L, mem, CHK, dtype) == {"planar", "interleaved", "elementwise"}


def test_clamp_and_count(L, mem):
    mc.case_clamp_and_count(L, mem, CHK)


def test_a_host_pointer_is_an_argument_error_not_a_fault(L, mem):
    """Ordinary host memory where an image or a destination is expected: GZ_E_ARG by the return code alone, on every
    entry; a good call afterwards still returns the right bits."""
    from guetzli_amd.capi import GZ_DT_F32, GZ_SAMPLES_LINEAR, device_map, device_output, device_pixels
    w, h = 33, 17
    a, b = blc.noise_pair(w, h)
    sa = blc.image_of_planes(a, "float32")
    host_out, host_plane = np.zeros((3, h, w), np.float32), np.zeros((h, w), np.float32)
    on_host = device_pixels(sa.ctypes.data, GZ_DT_F32, (3 * w, 3, 1))
    out_on_host = device_output(host_out.ctypes.data, GZ_DT_F32, (w, 1, w * h))
    map_on_host = device_map(host_plane.ctypes.data, GZ_DT_F32, (w, 1))
    good, held = blc.pixels_of(mem, dic.lay_out(sa, "float32", "HWC"))
    xyb, m, q = mc.Out(mem, w, h), mc.Out(mem, w, h), mc.QuantOut(mem, w, h)
    lib = L.lib
    assert lib.gz_opsin_device(0, w, h, C.byref(on_host), GZ_SAMPLES_LINEAR, 1.0, C.byref(xyb.arg), None) == -1
    assert lib.gz_opsin_device(0, w, h, C.byref(good), GZ_SAMPLES_LINEAR, 1.0, C.byref(out_on_host), None) == -1
    assert lib.gz_mask_device(0, w, h, C.byref(on_host), None, GZ_SAMPLES_LINEAR, 1.0, C.byref(m.arg), None, None) == -1
    assert lib.gz_mask_device(0, w, h, C.byref(good), C.byref(on_host), GZ_SAMPLES_LINEAR, 1.0, C.byref(m.arg), None, None) == -1
    assert lib.gz_mask_device(0, w, h, C.byref(good), None, GZ_SAMPLES_LINEAR, 1.0, C.byref(out_on_host), None, None) == -1
    assert lib.gz_mask_device(0, w, h, C.byref(good), None, GZ_SAMPLES_LINEAR, 1.0, C.byref(m.arg), C.byref(out_on_host), None) == -1
    assert lib.gz_adaptive_quantization(0, w, h, C.byref(on_host), 1.0, C.byref(q.arg), None) == -1
    assert lib.gz_adaptive_quantization(0, w, h, C.byref(good), 1.0, C.byref(map_on_host), None) == -1
    assert not host_out.any() and not host_plane.any()
    xyb.untouched("refused calls")
    m.untouched("refused calls")
    L.opsin_device(good, w, h, xyb.arg, GZ_SAMPLES_LINEAR)
    xyb.check(mc.expected_opsin(CHK, a), "opsin image after the refusals")
    L.mask_device(good, None, w, h, m.arg, None, GZ_SAMPLES_LINEAR)
    m.check(mc.expected_mask(CHK, a, a)[0], "mask after the refusals")
    L.adaptive_quantization(good, w, h, q.arg)
    q.check(mc.expected_quant(CHK, a), "quantisation field after the refusals")


# ------------------------------------------------------------------ the Python API on torch tensors ----
def test_the_three_functions_on_torch_tensors(torch):
    import guetzli_amd
    w, h = 33, 17
    a, b = blc.noise_pair(w, h)
    em, edc = mc.expected_mask(CHK, a, b)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    xyb = guetzli_amd.opsin_dynamics(ta, linear=True)
    assert xyb.is_cuda and xyb.dtype == torch.float32 and tuple(xyb.shape) == (3, h, w)
    assert_bits_equal(xyb.cpu().numpy(), mc.expected_opsin(CHK, a), "opsin_dynamics")
    m, dc = guetzli_amd.mask(ta, tb, dc=True, linear=True)
    assert_bits_equal(m.cpu().numpy(), em, "mask")
    assert_bits_equal(dc.cpu().numpy(), edc, "mask_dc")
    assert_bits_equal(guetzli_amd.mask(ta, linear=True, layout="HWC").cpu().numpy(), mc.expected_mask(CHK, a, a)[0].transpose(1, 2, 0), "mask of one image, HWC")
    # [0, 1] data with scale=255
    a01 = a / np.float32(255)
    q = guetzli_amd.adaptive_quantization(torch.from_numpy(a01).cuda(), scale=255)
    assert q.is_cuda and q.dtype == torch.float32 and tuple(q.shape) == (h, w)
    assert_bits_equal(q.cpu().numpy(), mc.expected_quant(CHK, a01 * np.float32(255)), "adaptive_quantization(scale=255)")
    # 8-bit tensors, as butteraugli() takes them
    rgb0, rgb1 = bpc.pair("photo", w, h)
    l0, l1 = blc.fields.linear(rgb0), blc.fields.linear(rgb1)
    got = guetzli_amd.mask(torch.from_numpy(rgb0).cuda(), torch.from_numpy(rgb1).cuda())
    assert_bits_equal(got.cpu().numpy(), mc.expected_mask(CHK, l0, l1)[0], "mask of uint8 tensors")
    assert_bits_equal(guetzli_amd.opsin_dynamics(rgb0).cpu().numpy(), mc.expected_opsin(CHK, l0), "opsin_dynamics of host bytes")
    # out= as crop views of larger tensors: a float16 plane, a bfloat16 HWC image
    canvas = torch.full((h + 5, w + 19), -7.0, dtype=torch.float16, device="cuda")
    view = canvas[3:3 + h, 8:8 + w]
    assert guetzli_amd.adaptive_quantization(ta, out=view) is view
    assert np.array_equal(view.contiguous().view(torch.int16).cpu().numpy().view(np.uint16), bpc.emitted_map(mc.expected_quant(CHK, a), "float16"))
    canvas[3:3 + h, 8:8 + w] = -7.0
    assert bool((canvas == -7.0).all())   # nothing around the crop was touched
    canvas3 = torch.full((h + 2, w + 7, 3), -7.0, dtype=torch.bfloat16, device="cuda")
    view3 = canvas3[1:1 + h, 3:3 + w]
    assert guetzli_amd.mask(ta, tb, linear=True, out=view3, layout="HWC") is view3
    want = bpc.emitted_map(np.ascontiguousarray(em.transpose(1, 2, 0)), "bfloat16")
    assert np.array_equal(view3.contiguous().view(torch.int16).cpu().numpy().view(np.uint16), want)
    canvas3[1:1 + h, 3:3 + w] = -7.0
    assert bool((canvas3 == -7.0).all())
    xview = torch.full((3, h + 2, w + 7), -7.0, device="cuda")
    assert_bits_equal(guetzli_amd.opsin_dynamics(ta, linear=True, out=xview[:, 1:1 + h, 3:3 + w]).cpu().numpy(), mc.expected_opsin(CHK, a), "opsin_dynamics(out=crop)")
    # strict=True on a clamped image; sizes the entries refuse
    bad = a.copy()
    bad[1, 2, 3] = np.nan
    bad[0, 0, 0] = 300
    tbad = torch.from_numpy(bad).cuda()
    guetzli_amd.adaptive_quantization(tbad)
    with pytest.raises(ValueError, match="2 elements"):
        guetzli_amd.adaptive_quantization(tbad, strict=True)
    with pytest.raises(ValueError, match="2 elements"):
        guetzli_amd.mask(tbad, tb, linear=True, strict=True)
    with pytest.raises(ValueError, match="16 x 16"):
        guetzli_amd.adaptive_quantization(ta[:, :16, :15])
    with pytest.raises(ValueError, match="8 x 8"):
        guetzli_amd.mask(ta[:, :7], linear=True)
    with pytest.raises(ValueError, match="device"):
        guetzli_amd.mask(ta, tb, linear=True, device=1)


def test_the_consumer_stream_sees_the_results(torch):
    """The three functions under a non-default stream that is busy, the image produced on that stream just before, a
    consumer enqueued on it right after: it reads the results, with no synchronisation in between."""
    import guetzli_amd
    w, h = 64, 17
    a, b = blc.noise_pair(w, h)
    busy = torch.ones((2048, 2048), device="cuda")
    staged = torch.from_numpy(a).cuda()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(8):
            busy = busy @ busy * 0.0 + 1.0
        image = torch.zeros((3, h, w), dtype=torch.float32, device="cuda")
        image.copy_(staged)                                   # the producer, on s
        q = torch.zeros((h, w), dtype=torch.float32, device="cuda")
        assert guetzli_amd.adaptive_quantization(image, out=q, stream=s.cuda_stream) is q      # stream= names it; the others find it current
        m = guetzli_amd.mask(image, linear=True)
        xyb = guetzli_amd.opsin_dynamics(image, linear=True)
        copies = [t.clone() for t in (q, m, xyb)]             # the consumers, on s
    torch.cuda.synchronize()
    assert_bits_equal(copies[0].cpu().numpy(), mc.expected_quant(CHK, a), "the field the consumer read")
    assert_bits_equal(copies[1].cpu().numpy(), mc.expected_mask(CHK, a, a)[0], "the mask the consumer read")
    assert_bits_equal(copies[2].cpu().numpy(), mc.expected_opsin(CHK, a), "the opsin image the consumer read")
