"""Butteraugli of linear float images on the MI355X: gz_create_from_device_linear / gz_set_linear_device /
gz_compare_device_linear / gz_butteraugli_linear on memory of torch tensors -- the cases of
tests/butteraugli_linear_cases.py, which tests/test_butteraugli_linear_emu.py runs through the CPU emulation -- and
guetzli_amd.butteraugli_linear / Comparator(linear=True) on torch tensors.  Here the 16-byte loads and stores, the
wavefront's vote and the atomics are the device's own.  Expectations come from the checkers under oracle/ (the CPU
restatement, and the unmodified reference behind oracle/_ref where it is built); every comparison is bitwise."""
import ctypes as C

import numpy as np
import pytest

import butteraugli_linear_cases as blc
import butteraugli_pair_cases as bpc
import device_input_cases as dic
import heatmap_cases as hc
from checkers import assert_bits_equal, bits, oracle, ref

pytestmark = pytest.mark.gpu

CHK = ref or oracle
GOOD, BAD = hc.default_thresholds()


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
def test_parity_of_linear_pairs_and_swapped(L, mem):
    blc.case_parity(L, mem, CHK)


def test_a_difference_under_a_byte_step_has_a_distance(L, mem):
    blc.case_the_byte_path_cannot_see_it(L, mem, CHK)


@pytest.mark.parametrize("dtype", blc.DTYPES)
def test_every_way_in(L, mem, dtype):
    assert blc.case_every_way_in(L, mem, CHK, dtype) == {"planar", "interleaved", "elementwise"}


def test_clamp_and_count(L, mem):
    blc.case_clamp_and_count(L, mem, CHK)


def test_small_images_take_the_references_border(L, mem):
    blc.case_small_images(L, mem, CHK, GOOD, BAD)


def test_state_of_a_linear_context(L, mem):
    blc.case_state(L, mem, CHK)


def test_a_pending_compare_refuses_linear_entries(L, mem):
    blc.case_pending_compare_refuses(L, mem)


def test_a_host_pointer_is_an_argument_error_not_a_fault(L, mem):
    """Ordinary host memory where a linear image is expected: GZ_E_ARG by the return code alone, on every new entry."""
    from guetzli_amd.capi import GZ_DT_F32, device_pixels
    w, h = 33, 17
    a, b = blc.noise_pair(w, h)
    sa = blc.image_of_planes(a, "float32")
    on_host = device_pixels(sa.ctypes.data, GZ_DT_F32, (3 * w, 3, 1))
    good, held = blc.pixels_of(mem, dic.lay_out(sa, "float32", "HWC"))
    dist = np.zeros(1, np.float32)
    err = C.c_int(0)
    assert not L.lib.gz_create_from_device_linear(0, w, h, C.byref(on_host), 1.0, C.byref(err)) and err.value == -1
    assert L.lib.gz_butteraugli_linear(0, w, h, C.byref(good), C.byref(on_host), 1.0, dist.ctypes.data, None, None, 0.0, 0.0, None) == -1
    assert L.lib.gz_butteraugli_linear(0, w, h, C.byref(on_host), C.byref(good), 1.0, dist.ctypes.data, None, None, 0.0, 0.0, None) == -1
    with L.context_from_device_linear(good, w, h) as ctx:
        assert L.lib.gz_compare_device_linear(ctx.handle, C.byref(on_host), 1.0, dist.ctypes.data, None, None, 0.0, 0.0, None) == -1
        assert L.lib.gz_set_linear_device(ctx.handle, C.byref(on_host), 1.0) == -1
        assert dist[0] == 0
        sb = blc.image_of_planes(b, "float32")
        d, m, _ = blc.compare_linear(ctx, mem, dic.lay_out(sb, "float32", "HWC"))
        assert bits(d) == bits(blc.expected(CHK, a, b)[0])


# ------------------------------------------------------------------ the Python API on torch tensors ----
def tensor_of(torch, storage, dtype):
    t = torch.from_numpy(np.ascontiguousarray(storage)).cuda()
    return t.view(torch.int16).view(getattr(torch, dtype)) if dtype in ("float16", "bfloat16") else t


def test_butteraugli_linear_of_torch_tensors(torch):
    import guetzli_amd
    w, h = 33, 17
    a, b = blc.noise_pair(w, h)
    a01, b01 = a / np.float32(255), b / np.float32(255)                     # [0, 1] data, CHW
    ea, eb = a01 * np.float32(255), b01 * np.float32(255)
    ed, em = blc.expected(CHK, ea, eb)
    ta, tb = torch.from_numpy(a01).cuda(), torch.from_numpy(b01).cuda()
    d = guetzli_amd.butteraugli_linear(ta, tb, scale=255)
    assert isinstance(d, float) and bits(np.float32(d)) == bits(ed) and d > 0
    d, m, heat = guetzli_amd.butteraugli_linear(ta, tb, scale=255, distmap=True, heatmap=True)
    assert m.is_cuda and m.dtype == torch.float32 and tuple(m.shape) == (h, w)
    assert bits(np.float32(d)) == bits(ed)
    assert_bits_equal(m.cpu().numpy(), em, "butteraugli_linear(distmap=True)")
    assert heat.dtype == torch.uint8 and np.array_equal(heat.cpu().numpy(), hc.expected_heat(em, GOOD, BAD))
    # HWC bfloat16 against a CHW float32 reference; the map into a float16 crop view
    s16 = blc.to_storage(np.ascontiguousarray(b.transpose(1, 2, 0)), "bfloat16")
    e16 = blc.planes_of(s16, "bfloat16")
    xd, xm = blc.expected(CHK, a, e16)
    canvas = torch.full((h + 5, w + 19), -7.0, dtype=torch.float16, device="cuda")
    view = canvas[3:3 + h, 8:8 + w]
    d, m = guetzli_amd.butteraugli_linear(torch.from_numpy(a).cuda(), tensor_of(torch, s16, "bfloat16"), distmap=view)
    assert m is view and bits(np.float32(d)) == bits(xd)
    assert np.array_equal(view.contiguous().view(torch.int16).cpu().numpy().view(np.uint16), bpc.emitted_map(xm, "float16"))
    canvas[3:3 + h, 8:8 + w] = -7.0
    assert bool((canvas == -7.0).all())   # nothing around the crop was touched
    # host arrays are uploaded first; 1 x 1 works
    assert bits(np.float32(guetzli_amd.butteraugli_linear(a, b))) == bits(blc.expected(CHK, a, b)[0])
    one0, one1 = np.float32([[[10.0, 200.0, 30.5]]]), np.float32([[[12.0, 190.0, 30.0]]])
    sd, sm = blc.expected_small(CHK, blc.planes_of(one0, "float32"), blc.planes_of(one1, "float32"))
    d, m = guetzli_amd.butteraugli_linear(torch.from_numpy(one0).cuda(), torch.from_numpy(one1).cuda(), distmap=True)
    assert bits(np.float32(d)) == bits(sd)
    assert_bits_equal(m.cpu().numpy(), sm, "1 x 1")
    # strict=True on a clamped image
    bad = a.copy()
    bad[1, 2, 3] = np.nan
    bad[0, 0, 0] = 300
    assert guetzli_amd.butteraugli_linear(torch.from_numpy(bad).cuda(), torch.from_numpy(b).cuda()) >= 0
    with pytest.raises(ValueError, match="2 elements"):
        guetzli_amd.butteraugli_linear(torch.from_numpy(bad).cuda(), torch.from_numpy(b).cuda(), strict=True)
    # refusals, before anything is computed
    with pytest.raises(ValueError, match="differ in size"):
        guetzli_amd.butteraugli_linear(ta, tb[:, :, :-1])
    with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
        guetzli_amd.butteraugli_linear(ta.to(torch.uint8), tb)
    with pytest.raises(ValueError, match="alpha is not supported"):
        guetzli_amd.butteraugli_linear(torch.zeros((h, w, 4), device="cuda"), torch.zeros((h, w, 4), device="cuda"))
    with pytest.raises(ValueError, match="device"):
        guetzli_amd.butteraugli_linear(ta, tb, device=1)


def test_a_linear_comparator_reused_for_three_images(torch):
    import guetzli_amd
    w, h = 33, 17
    a, b = blc.noise_pair(w, h)
    with guetzli_amd.Comparator(torch.from_numpy(a).cuda(), linear=True) as cmp:
        for k in range(3):
            other = np.clip(b + np.float32(0.25 * k), 0, 255).astype(np.float32)
            ed, em = blc.expected(CHK, a, other)
            d, m = cmp.compare(torch.from_numpy(other).cuda(), distmap=True)
            assert bits(np.float32(d)) == bits(ed), k
            assert_bits_equal(m.cpu().numpy(), em, f"image {k}")
            assert cmp.clamped == 0
        over = b.copy()
        over[2, 5, 7] = -3
        cmp.compare(torch.from_numpy(over).cuda())
        assert cmp.clamped == 1


def test_the_consumer_stream_sees_the_map(torch):
    """compare(distmap=tensor) of a linear Comparator under a non-default stream that is busy, the distorted image
    produced on that stream just before, a consumer enqueued on it right after: it reads the map, with no
    synchronisation in between."""
    import guetzli_amd
    w, h = 64, 17
    a, b = blc.noise_pair(w, h)
    ed, em = blc.expected(CHK, a, b)
    busy = torch.ones((2048, 2048), device="cuda")
    staged = torch.from_numpy(b).cuda()
    s = torch.cuda.Stream()
    with guetzli_amd.Comparator(torch.from_numpy(a).cuda(), linear=True) as cmp:
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(8):
                busy = busy @ busy * 0.0 + 1.0
            other = torch.zeros((3, h, w), dtype=torch.float32, device="cuda")
            other.copy_(staged)                                   # the producer, on s
            out = torch.zeros((h, w), dtype=torch.float32, device="cuda")
            d, m = cmp.compare(other, distmap=out)
            copy = out.clone()                                    # the consumer, on s
        torch.cuda.synchronize()
    assert m is out and bits(np.float32(d)) == bits(ed)
    assert_bits_equal(copy.cpu().numpy(), em, "the map the consumer read")
