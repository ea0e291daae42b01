"""The image-pair metric on the MI355X: gz_compare_device_pixels / gz_compare_rgb / gz_distmap_device / gz_probe_emit_map
on memory of torch tensors -- the cases of tests/butteraugli_pair_cases.py, which tests/test_butteraugli_pair_emu.py runs
through the CPU emulation -- and guetzli_amd.butteraugli / Comparator on torch tensors.  Here the 16-byte loads and
stores and the 16-bit roundings are the device's own.  Expectations come from the checkers under oracle/ (the CPU
restatement, and the unmodified reference behind oracle/_ref where it is built); every comparison is bitwise."""
import ctypes as C

import numpy as np
import pytest

import butteraugli_pair_cases as bpc
import device_input_cases as dic
import device_output_cases as doc
import images
from checkers import assert_bits_equal, bits, oracle, ref

pytestmark = pytest.mark.gpu

CHK = ref or oracle
TARGET = 0.971769
CONFIG_IDS = ["patch2_ahead", "three_streams", "one_stream"]


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
def test_pair_parity_at_every_size(L, mem):
    bpc.case_pair_parity_every_size(L, mem, CHK)


def test_pair_parity_of_every_pair_and_swapped(L, mem):
    bpc.case_pair_parity_every_pair(L, mem, CHK)


@pytest.mark.parametrize("dtype", bpc.dac.DTYPES)
def test_every_way_in(L, mem, dtype):
    bpc.case_every_way_in(L, mem, CHK, dtype)


@pytest.mark.parametrize("layout", bpc.MAP_LAYOUTS)
@pytest.mark.parametrize("dtype", bpc.MAP_DTYPES)
def test_map_emit_alone(L, mem, dtype, layout):
    bpc.case_map_emit_alone(L, mem, dtype, layout)


@pytest.mark.parametrize("dtype", bpc.MAP_DTYPES)
def test_rounding_over_the_float32_domain(L, mem, dtype):
    bpc.case_rounding(L, mem, dtype)


@pytest.mark.parametrize("frame", [1, 2])
@pytest.mark.parametrize("config", bpc.CONFIGS, ids=CONFIG_IDS)
def test_state_around_a_pixel_comparison(L, mem, config, frame):
    bpc.case_state(L, mem, CHK, config, frame)


def test_distmap_device_follows_the_last_stored_map(L, mem):
    bpc.case_distmap_device(L, mem)


def test_a_pending_compare_refuses_pixel_comparisons(L, mem):
    bpc.case_pending_compare_refuses(L, mem)


# ------------------------------------------------------------------ arguments, streams ----
def test_a_host_pointer_is_an_argument_error_not_a_fault(torch, L, mem):
    """Ordinary host memory where device memory is expected -- the other image, or the map: GZ_E_ARG (by the return code
    alone), nothing is written, and the context goes on working."""
    from guetzli_amd.capi import GZ_DT_F32, GZ_DT_U8, device_map, device_pixels
    w, h = 33, 17
    rgb0, rgb1 = bpc.pair("photo", w, h)
    ed, em = bpc.expected(CHK, rgb0, rgb1)
    host_map = np.zeros((h, w), np.float32)
    dist = np.zeros(1, np.float32)
    plane = np.ones((h, w), np.float32)
    on_host = device_map(host_map.ctypes.data, GZ_DT_F32, (w, 1))
    assert L.lib.gz_probe_emit_map(0, plane.ctypes.data, w, h, C.byref(on_host)) == -1
    with L.context(rgb0, TARGET) as ctx:
        ctx.encode_rgb(download=False)
        ctx.quantize(bpc.Q, download=False)
        exp = ctx.compare()
        good, held = bpc.pixels_of(mem, dic.lay_out(rgb1, "uint8", "HWC"))
        assert L.lib.gz_compare_device_pixels(ctx.handle, C.byref(good), dist.ctypes.data, C.byref(on_host)) == -1
        assert L.lib.gz_distmap_device(ctx.handle, C.byref(on_host)) == -1
        bad = device_pixels(rgb1.ctypes.data, GZ_DT_U8, (3 * w, 3, 1))
        assert L.lib.gz_compare_device_pixels(ctx.handle, C.byref(bad), dist.ctypes.data, None) == -1
        assert not host_map.any() and dist[0] == 0
        got = ctx.compare()
        for g, e in zip(got, exp):
            assert_bits_equal(np.asarray(g, np.float32), np.asarray(e, np.float32), "gz_compare after the refusals")
        d, m = bpc.compare_pixels(ctx, mem, dic.lay_out(rgb1, "uint8", "HWC"), w, h)
        assert bits(d) == bits(ed)
        assert_bits_equal(m, em, "map")


def test_the_consumer_stream_sees_the_map(torch):
    """compare(distmap=tensor) under a non-default stream that is busy, the distorted image produced on that stream
    just before, a consumer enqueued on it right after: it reads the map, with no synchronisation in between."""
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
            out = torch.zeros((h, w), dtype=torch.float32, device="cuda")
            d, m = cmp.compare(other, distmap=out)
            copy = out.clone()                                    # the consumer, on s
        torch.cuda.synchronize()
    assert m is out and bits(np.float32(d)) == bits(ed)
    assert_bits_equal(copy.cpu().numpy(), em, "the map the consumer read")


# ------------------------------------------------------------------ butteraugli() and Comparator on torch tensors ----
def tensor_of(torch, rgb, dtype, layout="HWC"):
    """A GPU tensor of `dtype` whose bytes, by the ingest rule, are `rgb`."""
    s = bpc.storage_of_bytes(rgb, dtype)
    t = torch.from_numpy(np.ascontiguousarray(s)).cuda()
    if dtype in ("float16", "bfloat16"):
        t = t.view(torch.int16).view(getattr(torch, dtype))
    return t.permute(2, 0, 1).contiguous() if layout == "CHW" else t


def test_butteraugli_of_torch_tensors(torch):
    import guetzli_amd
    w, h = 61, 17
    for name in bpc.PAIRS:
        rgb0, rgb1 = bpc.pair(name, w, h)
        ed, em = bpc.expected(CHK, rgb0, rgb1)
        d = guetzli_amd.butteraugli(torch.from_numpy(rgb0).cuda(), torch.from_numpy(rgb1).cuda())
        assert isinstance(d, float) and bits(np.float32(d)) == bits(ed), name
        d, m = guetzli_amd.butteraugli(torch.from_numpy(rgb0).cuda(), torch.from_numpy(rgb1).cuda(), distmap=True)
        assert m.is_cuda and m.dtype == torch.float32 and tuple(m.shape) == (h, w)
        assert bits(np.float32(d)) == bits(ed)
        assert_bits_equal(m.cpu().numpy(), em, name)
    rgb0, rgb1 = bpc.pair("photo", w, h)
    ed, em = bpc.expected(CHK, rgb0, rgb1)
    for dt0, dt1, layout in (("float32", "bfloat16", "CHW"), ("uint16", "float16", "HWC"), ("float16", "uint8", "CHW")):
        d, m = guetzli_amd.butteraugli(tensor_of(torch, rgb0, dt0, layout), tensor_of(torch, rgb1, dt1, layout), distmap=True)
        assert bits(np.float32(d)) == bits(ed), (dt0, dt1)
        assert_bits_equal(m.cpu().numpy(), em, f"{dt0} against {dt1}")
    # host pixels on either side
    assert bits(np.float32(guetzli_amd.butteraugli(rgb0, rgb1))) == bits(ed)
    d, m = guetzli_amd.butteraugli(rgb0, torch.from_numpy(rgb1).cuda(), distmap=True)
    assert bits(np.float32(d)) == bits(ed)
    assert_bits_equal(m.cpu().numpy(), em, "host reference, device distorted")
    d, m = guetzli_amd.butteraugli(torch.from_numpy(rgb0).cuda(), rgb1, distmap=True)
    assert m.is_cuda and bits(np.float32(d)) == bits(ed)
    assert_bits_equal(m.cpu().numpy(), em, "device reference, host distorted")
    # RGBA over a background that is not black
    rgba = np.concatenate([rgb1, images.noise(w, h, seed=9)[:, :, :1]], -1)
    blended = guetzli_amd.blend_on_background(rgba, bpc.BACKGROUND)
    d = guetzli_amd.butteraugli(torch.from_numpy(rgb0).cuda(), torch.from_numpy(rgba).cuda(), background=bpc.BACKGROUND)
    assert bits(np.float32(d)) == bits(bpc.expected(CHK, rgb0, blended)[0])


def test_comparator_fills_a_crop_view(torch):
    """One reference, several distorted images; a crop-view distmap= inside a sentinel canvas, of each map dtype."""
    import guetzli_amd
    w, h = 61, 17
    rgb0, _ = bpc.pair("photo", w, h)
    with guetzli_amd.Comparator(torch.from_numpy(rgb0).cuda()) as cmp:
        for name, dtype in zip(bpc.PAIRS, ("float32", "float16", "bfloat16", "float32")):
            other = bpc.pair(name, w, h)[1]
            ed, em = bpc.expected(CHK, rgb0, other)
            canvas = torch.full((h + 5, w + 19), -7.0, dtype=getattr(torch, dtype), device="cuda")
            view = canvas[3:3 + h, 8:8 + w]
            d, m = cmp.compare(torch.from_numpy(other).cuda(), distmap=view)
            assert m is view and bits(np.float32(d)) == bits(ed), name
            got = view.contiguous()
            got = got.cpu().numpy() if dtype == "float32" else got.view(torch.int16).cpu().numpy().view(np.uint16)
            exp = bpc.emitted_map(em, dtype)
            assert np.array_equal(got.view(np.uint32) if dtype == "float32" else got, exp.view(np.uint32) if dtype == "float32" else exp), (name, dtype)
            canvas[3:3 + h, 8:8 + w] = -7.0
            assert bool((canvas == -7.0).all())   # nothing around the crop was touched
            assert bits(np.float32(cmp.compare(other))) == bits(ed)


def coefficients_of(jpeg):
    """The dequantised coefficients of a JPEG of this library's writer, by its own reader (gzh_read_jpeg's dump)."""
    import guetzli_amd
    lib = guetzli_amd.load_host().lib
    lib.gzh_read_jpeg.restype = C.c_long
    lib.gzh_read_jpeg.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    buf = np.frombuffer(jpeg, np.uint8)
    out = np.zeros(1 << 24, np.uint8)
    n = lib.gzh_read_jpeg(buf.ctypes.data, len(jpeg), out.ctypes.data, out.size)
    assert 0 < n <= out.size
    return doc.frame_of_dump(doc.parse_jpeg_dump(out[:n].tobytes()))


def test_the_distance_of_an_encode_from_its_original(torch):
    """butteraugli(rgb, decode(process(rgb)[0])) is the comparator's distance of that JPEG's coefficients: the number the
    search accepted the output for."""
    import guetzli_amd
    w, h = 61, 43
    rgb = images.crop(w, h, 50, 40)
    t = torch.from_numpy(rgb).cuda()
    jpeg, _ = guetzli_amd.process(t, target=TARGET)
    co, factor = coefficients_of(jpeg)
    assert factor == 1
    oc = CHK.comparator(rgb, TARGET)
    ed, em = oc.compare(co)
    oc.close()
    d, m = guetzli_amd.butteraugli(t, guetzli_amd.decode(jpeg), distmap=True)
    assert bits(np.float32(d)) == bits(np.float32(ed))
    assert_bits_equal(m.cpu().numpy(), em, "map of the encode")


def test_butteraugli_refuses(torch):
    import guetzli_amd
    w, h = 33, 17
    rgb0, rgb1 = bpc.pair("photo", w, h)
    t0, t1 = torch.from_numpy(rgb0).cuda(), torch.from_numpy(rgb1).cuda()
    with pytest.raises(ValueError, match="differ in size"):
        guetzli_amd.butteraugli(t0, t1[:, :-1])
    with pytest.raises(ValueError, match="8 x 8"):
        guetzli_amd.butteraugli(t0[:7], t1[:7])
    with pytest.raises(ValueError, match="device"):
        guetzli_amd.butteraugli(t0, t1, device=1)
    with pytest.raises(ValueError, match="share an address"):
        guetzli_amd.butteraugli(t0, t1, distmap=torch.zeros((h, 1), device="cuda").expand(h, w))
    with pytest.raises(ValueError, match="shape"):
        guetzli_amd.butteraugli(t0, t1, distmap=torch.zeros((w, h), device="cuda"))
    with pytest.raises(TypeError):
        guetzli_amd.butteraugli(t0, t1, distmap=torch.zeros((h, w), dtype=torch.float64, device="cuda"))
    with pytest.raises(TypeError):
        guetzli_amd.butteraugli(t0, t1, distmap=np.zeros((h, w), np.float32))
    with guetzli_amd.Comparator(t0) as cmp:
        with pytest.raises(ValueError, match="differ in size"):
            cmp.compare(t1[:-1])
        assert bits(np.float32(cmp.compare(t1))) == bits(bpc.expected(CHK, rgb0, rgb1)[0])
