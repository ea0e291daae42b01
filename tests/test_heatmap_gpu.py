"""Butteraugli's heat map on the MI355X: gz_probe_emit_heat / gz_heatmap_from_map_device / gz_heatmap_device /
gz_compare_device_pixels_heat on memory of torch tensors -- the cases of tests/heatmap_cases.py, which
tests/test_heatmap_emu.py runs through the CPU emulation -- and guetzli_amd.heatmap / butteraugli / Comparator on torch
tensors.  Here the FP64 arithmetic, the division, the LDS table and the 16-byte stores are the device's own.
Expectations are the restatement of ScoreToRgb in tests/heatmap_cases.py (pinned to the reference by
tests/test_heatmap_reference.py) and the reference's recorded output under tests/golden/heatmap; every comparison is
for equality.  No plane is larger than 67 x 17."""
import ctypes as C

import numpy as np
import pytest

import butteraugli_pair_cases as bpc
import device_output_cases as doc
import heatmap_cases as hc
from checkers import assert_bits_equal, bits, oracle, ref

pytestmark = pytest.mark.gpu

CHK = ref or oracle
GOOD, BAD = hc.default_thresholds()
THRESHOLDS = [pytest.param((GOOD, BAD), id="default"), pytest.param(hc.OTHER_THRESHOLDS, id="other")]
EXPECTED_PATHS = {"HWC": {"interleaved", "elementwise"}, "CHW": {"planar", "elementwise"}, "HWC_crop": {"interleaved"},
                  "CHW_crop": {"planar"}, "HWC_base1": {"elementwise"}, "CHW_crop_base1": {"elementwise"},
                  "HWC_pitch1": {"interleaved", "elementwise"}, "WHC": {"elementwise"}}


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
def test_the_device_library_has_the_hosts_table_and_thresholds(L):
    import math
    thr = L.probe_heat_thresholds()
    assert (np.diff(thr) > 0).all()
    for k in range(1, 256):   # thr[k] is the least double whose byte, by this process's pow, is k
        at, below = float(thr[k - 1]), math.nextafter(float(thr[k - 1]), 0.0)
        assert (int(255 * math.pow(at, 0.5) + 0.5), int(255 * math.pow(below, 0.5) + 0.5)) == (k, k - 1), k
    assert L.default_heat_thresholds() == (GOOD, BAD)


@pytest.mark.parametrize("thresholds", THRESHOLDS)
def test_every_synthetic_distance(L, mem, thresholds):
    hc.case_probe_values(L, mem, *thresholds)


def test_the_references_recorded_heat_map(L, mem):
    hc.case_golden(L, mem, GOOD, BAD)


@pytest.mark.parametrize("layout", hc.LAYOUTS)
@pytest.mark.parametrize("dtype", hc.DTYPES)
def test_probe_at_every_shape(L, mem, dtype, layout):
    paths = hc.case_probe_shapes(L, mem, dtype, layout, GOOD, BAD)
    assert paths == EXPECTED_PATHS[layout], paths


@pytest.mark.parametrize("layout", hc.LAYOUTS)
@pytest.mark.parametrize("dtype", ["uint8", "float32", "bfloat16"])
def test_the_context_free_entry_at_every_shape(L, mem, dtype, layout):
    hc.case_from_map_shapes(L, mem, dtype, layout, GOOD, BAD)


def test_compare_with_a_heat_map(L, mem):
    hc.case_compare_with_heat(L, mem, CHK, GOOD, BAD)


def test_heatmap_device_follows_the_last_stored_map(L, mem):
    hc.case_state(L, mem, GOOD, BAD)


# ------------------------------------------------------------------ arguments, streams ----
def test_a_host_pointer_is_an_argument_error_not_a_fault(torch, L, mem):
    """Ordinary host memory where device memory is expected -- the heat map's destination, or the caller's map: GZ_E_ARG,
    nothing is written, and the context goes on working."""
    from guetzli_amd.capi import GZ_DT_U8, device_output
    w, h = 33, 17
    rgb0, rgb1 = bpc.pair("photo", w, h)
    ed, em = bpc.expected(CHK, rgb0, rgb1)
    host_heat = np.zeros((h, w, 3), np.uint8)
    plane = np.ones((h, w), np.float32)
    dist = np.zeros(1, np.float32)
    on_host = device_output(host_heat.ctypes.data, GZ_DT_U8, (3 * w, 3, 1))
    on_device = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    good_out = device_output(on_device.data_ptr(), GZ_DT_U8, (3 * w, 3, 1))
    assert L.lib.gz_probe_emit_heat(0, plane.ctypes.data, w, h, GOOD, BAD, C.byref(on_host)) == -1
    assert L.lib.gz_heatmap_from_map_device(0, plane.ctypes.data, w, h, w, GOOD, BAD, C.byref(good_out)) == -1    # the map on the host
    # ... or leaving its allocation.  (The library sees the HIP allocation, which under torch's caching allocator is the
    # whole segment a tensor was cut from: the extent has to leave that -- rows 64 MB apart do.)
    short = torch.ones((h * w,), device="cuda")
    assert L.lib.gz_heatmap_from_map_device(0, short.data_ptr(), w, h, 1 << 24, GOOD, BAD, C.byref(good_out)) == -1
    assert L.lib.gz_heatmap_from_map_device(0, short.data_ptr(), w, h, w, GOOD, BAD, C.byref(good_out)) == 0
    assert np.array_equal(on_device.cpu().numpy(), hc.expected_heat(plane, GOOD, BAD))
    on_device.zero_()
    with L.context(rgb0, bpc.TARGET) as ctx:
        px, held = bpc.pixels_of(mem, bpc.dic.lay_out(rgb1, "uint8", "HWC"))
        assert L.lib.gz_compare_device_pixels_heat(ctx.handle, C.byref(px), dist.ctypes.data, None, C.byref(on_host), GOOD, BAD) == -1
        ctx.compare_rgb(rgb1)
        assert L.lib.gz_heatmap_device(ctx.handle, GOOD, BAD, C.byref(on_host)) == -1
        assert not host_heat.any() and dist[0] == 0 and not bool(on_device.any())
        d = ctx.compare_device_pixels_heat(px, good_out, GOOD, BAD)
        assert bits(np.float32(d)) == bits(ed)
        assert np.array_equal(on_device.cpu().numpy(), hc.expected_heat(em, GOOD, BAD))


def test_the_consumer_stream_sees_the_heat_map(torch):
    """compare(heatmap=tensor) under a non-default stream that is busy, the distorted image produced on that stream
    just before, a consumer enqueued on it right after: it reads the picture, with no synchronisation in between;
    then heatmap() of the map on the same stream."""
    import guetzli_amd
    w, h = 64, 17
    rgb0, rgb1 = bpc.pair("photo", w, h)
    ed, em = bpc.expected(CHK, rgb0, rgb1)
    busy = torch.ones((2048, 2048), device="cuda")
    staged = torch.from_numpy(rgb1).cuda()
    s = torch.cuda.Stream()
    with guetzli_amd.Comparator(torch.from_numpy(rgb0).cuda()) as cmp:
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(8):
                busy = busy @ busy * 0.0 + 1.0
            other = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
            other.copy_(staged)                                   # the producer, on s
            out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
            d, m, hm = cmp.compare(other, distmap=True, heatmap=out)
            copy = out.clone()                                    # the consumer, on s
            again = guetzli_amd.heatmap(m * 1.0).clone()          # a map produced on s, its picture read on s
        torch.cuda.synchronize()
    assert hm is out and bits(np.float32(d)) == bits(ed)
    heat = hc.expected_heat(em, GOOD, BAD)
    assert np.array_equal(copy.cpu().numpy(), heat)
    assert np.array_equal(again.cpu().numpy(), heat)


# ------------------------------------------------------------------ the Python surface on torch tensors ----
def test_the_python_surface(torch):
    import guetzli_amd
    w, h = 67, 9
    rgb0, rgb1 = bpc.pair("photo", w, h)
    ed, em = bpc.expected(CHK, rgb0, rgb1)
    heat = hc.expected_heat(em, GOOD, BAD)
    t0, t1 = torch.from_numpy(rgb0).cuda(), torch.from_numpy(rgb1).cuda()
    assert guetzli_amd.fuzzy_inverse(1.5) == GOOD and guetzli_amd.fuzzy_inverse(0.5) == BAD
    assert guetzli_amd.fuzzy_class(GOOD) == hc.fuzzy_class(GOOD)
    # without heatmap=, return values are what they were
    assert isinstance(guetzli_amd.butteraugli(t0, t1), float)
    assert len(guetzli_amd.butteraugli(t0, t1, distmap=True)) == 2
    d, hm = guetzli_amd.butteraugli(t0, t1, heatmap=True)
    assert hm.is_cuda and hm.dtype == torch.uint8 and tuple(hm.shape) == (h, w, 3)
    assert bits(np.float32(d)) == bits(ed) and np.array_equal(hm.cpu().numpy(), heat)
    d, m, hm = guetzli_amd.butteraugli(rgb0, t1, distmap=True, heatmap=True)        # a host reference
    assert np.array_equal(hm.cpu().numpy(), heat)
    assert_bits_equal(m.cpu().numpy(), em, "the map beside the heat map")
    d, hm = guetzli_amd.butteraugli(t0, rgb1, heatmap=True)                         # host distorted pixels
    assert bits(np.float32(d)) == bits(ed) and np.array_equal(hm.cpu().numpy(), heat)
    # a crop view of float16 in CHW inside a sentinel canvas, other thresholds
    canvas = torch.full((3, h + 5, w + 19), -7.0, dtype=torch.float16, device="cuda")
    view = canvas[:, 3:3 + h, 8:8 + w]
    with guetzli_amd.Comparator(t0) as cmp:
        d, hm = cmp.compare(t1, heatmap=view, good=0.5, bad=2.25)
        assert hm is view and bits(np.float32(d)) == bits(ed)
        got = view.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
        assert np.array_equal(got, doc.emitted(hc.expected_heat(em, 0.5, 2.25), "float16").transpose(2, 0, 1))
        canvas[:, 3:3 + h, 8:8 + w] = -7.0
        assert bool((canvas == -7.0).all())   # nothing around the crop was touched
        assert isinstance(cmp.compare(t1), float)
    # heatmap() of a map tensor: contiguous, a crop with a pitch, transposed (made contiguous in x), every dtype
    mt = torch.from_numpy(np.array(em)).cuda()   # (a writable copy: the expectation is handed out read-only)
    assert np.array_equal(guetzli_amd.heatmap(mt).cpu().numpy(), heat)
    wide = torch.zeros((h, w + 5), device="cuda")
    wide[:, 2:2 + w] = mt
    assert np.array_equal(guetzli_amd.heatmap(wide[:, 2:2 + w], dtype="uint16", layout="CHW").cpu().numpy().astype(np.int64),
                          heat.transpose(2, 0, 1).astype(np.int64) * 257)
    assert np.array_equal(guetzli_amd.heatmap(mt.t().contiguous().t()).cpu().numpy(), heat)
    f = guetzli_amd.heatmap(mt, dtype="float32", good=0.5, bad=2.25)
    assert np.array_equal(f.cpu().numpy().view(np.uint32), doc.emitted(hc.expected_heat(em, 0.5, 2.25), "float32").view(np.uint32))
    # refusals
    with pytest.raises(ValueError, match="good"):
        guetzli_amd.heatmap(mt, good=1.0, bad=1.0)
    with pytest.raises(TypeError):
        guetzli_amd.heatmap(mt.double())
    with pytest.raises(ValueError, match="share an address"):
        guetzli_amd.butteraugli(t0, t1, heatmap=torch.zeros((h, 1, 3), dtype=torch.uint8, device="cuda").expand(h, w, 3))
    with pytest.raises(ValueError, match="shape"):
        guetzli_amd.butteraugli(t0, t1, heatmap=torch.zeros((w, h, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        guetzli_amd.butteraugli(t0, t1, heatmap=np.zeros((h, w, 3), np.uint8))
