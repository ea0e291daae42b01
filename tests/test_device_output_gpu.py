"""Device-resident output on the MI355X: gz_decode_coeffs_device / gz_reconstruct_device into memory of torch tensors,
guetzli_amd.decode and process(decoded=).  Here the 16-byte stores, the LDS table and the 16-bit roundings are the device's
own; the same cases run through the CPU emulation in tests/test_device_output_emu.py.  Expectations come from the
checkers under oracle/ (the CPU restatement, and the unmodified reference behind oracle/_ref where it is built)."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import device_input_cases as dic
import device_output_cases as doc
import images
from checkers import oracle, ref

pytestmark = pytest.mark.gpu

TARGET = 0.971769
# the reference's output for tests/golden/bees.png at quality 95 (tests/test_gpu_parity.py: GOLDEN_JPEG_SHA[(444, 258, 95)])
BEES_Q95_SHA = "f2673f12a4856e020627fa151493a80b1cb2ee4dc81e28afc62dc089baf50242"
SIZES = [(1, 1), (7, 5), (8, 8), (17, 9), (33, 31), (61, 43)]
CHK = ref or oracle


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def L():
    import guetzli_amd
    return guetzli_amd.load()


class OnDevice:
    """A doc.Destination whose buffer, sentinel included, lives on the GPU."""

    def __init__(self, torch, dest):
        self.dest = dest
        self.t = torch.from_numpy(dest.raw).cuda()
        assert self.t.data_ptr() % 64 == 0

    def output(self, stream=0):
        from guetzli_amd.capi import device_output
        from guetzli_amd.encoder import DTYPE_CODES
        d = self.dest
        return device_output(self.t.data_ptr() + d.offset * d.itemsize, DTYPE_CODES[d.dtype], d.strides, stream)

    def check(self, rgb, what=""):
        self.dest.check(rgb, raw=self.t.cpu().numpy(), what=what)


def sha(b):
    return hashlib.sha256(b).hexdigest()


# ------------------------------------------------------------------ emit parity, sentinels ----
@pytest.fixture(scope="module")
def decoded_cases():
    """Coefficients and their pixels (OutputImage::ToSRGB by the checker) for every width x height, computed once."""
    out = {}
    for h in doc.HEIGHTS:
        for w in doc.WIDTHS:
            co = doc.random_coeffs(w, h, 1, seed=1000 * h + w)
            out[(w, h)] = (co, CHK.reconstruct(co, w, h)[1])
    return out


@pytest.mark.parametrize("layout", doc.LAYOUTS)
@pytest.mark.parametrize("dtype", doc.DTYPES)
def test_emit_parity_and_untouched_neighbours(torch, L, decoded_cases, dtype, layout):
    for (w, h), (co, rgb) in decoded_cases.items():
        d = OnDevice(torch, doc.destination(w, h, dtype, layout))
        L.decode_coeffs_device(co, w, h, d.output())
        d.check(rgb, what=layout)


@pytest.mark.parametrize("dtype", doc.DTYPES)
def test_all_256_bytes_round_trip_through_the_ingest_kernel(torch, L, dtype):
    from guetzli_amd.capi import device_image, device_pixels
    from guetzli_amd.encoder import DTYPE_CODES
    co, w, h = doc.all_bytes_coeffs(lambda c, ww, hh: oracle.reconstruct(c, ww, hh)[1])
    rgb = L.decode_coeffs(co, w, h)
    assert set(np.unique(rgb).tolist()) == set(range(256))
    assert np.array_equal(rgb, CHK.reconstruct(co, w, h)[1])
    for layout in ("HWC", "CHW", "HWC_base1"):
        d = OnDevice(torch, doc.destination(w, h, dtype, layout))
        L.decode_coeffs_device(co, w, h, d.output())
        d.check(rgb)
        o = d.output()
        image = (device_pixels if dtype == "uint16" else device_image)(o.data, DTYPE_CODES[dtype], d.dest.strides)
        assert np.array_equal(L.pack_rgb_device(image, w, h), rgb), (dtype, layout)


# ------------------------------------------------------------------ decode against the reference ----
def frames(w, h, factor):
    yield "random", doc.random_coeffs(w, h, factor, seed=7 * w + h)
    co = oracle.encode_rgb(images.crop(w, h, 120, 80))
    if factor == 1:
        yield "bees", co
    elif w >= 8 and h >= 8:
        yield "bees", oracle.downsample(co, w, h)


@pytest.mark.parametrize("factor", [1, 2])
def test_decode_coeffs_is_to_srgb_of_the_reference(torch, L, factor):
    for w, h in SIZES:
        for name, co in frames(w, h, factor):
            exp = (CHK.reconstruct if factor == 1 else CHK.reconstruct420)(co, w, h)[1]
            got = L.decode_coeffs(co, w, h, factor)
            assert np.array_equal(got, exp), (name, w, h, factor, np.argwhere(got != exp)[:4])
            d = OnDevice(torch, doc.destination(w, h, "uint8", "HWC_crop"))
            L.decode_coeffs_device(co, w, h, d.output(), chroma_factor=factor)
            d.check(exp, what=name)


def test_reconstruct_device_is_reconstruct(torch, L):
    w, h = 61, 43
    rgb = images.crop(w, h, 50, 40)
    q = np.full((3, 64), 5, np.int32)
    s = torch.cuda.Stream()
    with L.context(rgb, 1.0) as ctx:
        ctx.encode_rgb()
        for frame in (1, 2):
            if frame == 2:
                ctx.downsample()
            ctx.quantize(q)
            exp = ctx.reconstruct()[0]
            for dtype, layout, stream in (("uint8", "HWC_crop", 0), ("bfloat16", "CHW", s.cuda_stream), ("float32", "WHC", 0)):
                d = OnDevice(torch, doc.destination(w, h, dtype, layout))
                torch.cuda.synchronize()
                ctx.reconstruct_device(d.output(stream))
                with torch.cuda.stream(s):
                    d.check(exp, what=(frame, dtype, layout))   # (its copy to the host runs on s, behind the event)


# ------------------------------------------------------------------ decode() of torch tensors ----
@pytest.fixture(scope="module")
def small_jpeg():
    """A 4:4:4 JPEG of 61 x 43 pixels and its decoded bytes."""
    import guetzli_amd
    host = guetzli_amd.load_host()
    w, h = 61, 43
    q = np.full((3, 64), 3, np.int32)
    co = (oracle.encode_rgb(images.crop(w, h, 30, 20)).astype(np.int32) // 3 * 3).astype(np.int16)
    return host.write_jpeg(co, w, h, q), CHK.reconstruct(co, w, h)[1]


def test_decode_allocates_a_tensor(torch, small_jpeg):
    import guetzli_amd
    jpeg, exp = small_jpeg
    t = guetzli_amd.decode(jpeg)
    assert t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (43, 61, 3)
    assert np.array_equal(t.cpu().numpy(), exp)
    assert np.array_equal(guetzli_amd.decode(jpeg, device="host"), exp)
    f = guetzli_amd.decode(jpeg, dtype=torch.float32, layout="CHW")
    assert tuple(f.shape) == (3, 43, 61) and np.array_equal(f.cpu().numpy(), doc.emitted(exp, "float32").transpose(2, 0, 1))
    assert guetzli_amd.process(f)[0] == guetzli_amd.process(exp)[0]   # the input side reads the same bytes back


def test_decode_into_a_bfloat16_chw_crop(torch, small_jpeg):
    import guetzli_amd
    jpeg, exp = small_jpeg
    canvas = torch.full((3, 43 + 10, 61 + 19), -7.0, dtype=torch.bfloat16, device="cuda")
    view = canvas[:, 5:5 + 43, 8:8 + 61]
    assert guetzli_amd.decode(jpeg, out=view, layout="CHW") is view
    got = view.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, doc.emitted(exp, "bfloat16").transpose(2, 0, 1))
    canvas[:, 5:5 + 43, 8:8 + 61] = -7.0
    assert bool((canvas == -7.0).all())   # nothing around the crop was touched


def test_decode_into_a_uint16_hwc_tensor(torch, small_jpeg):
    import guetzli_amd
    jpeg, exp = small_jpeg
    canvas = torch.from_numpy(np.full((43 + 3, 61 + 16, 3), 0x1234, np.uint16)).cuda()
    view = canvas[2:2 + 43, 16:16 + 61]
    guetzli_amd.decode(jpeg, out=view)
    back = canvas.cpu().numpy()
    assert np.array_equal(back[2:2 + 43, 16:16 + 61], exp.astype(np.uint16) * 257)
    back[2:2 + 43, 16:16 + 61] = 0x1234
    assert (back == 0x1234).all()


def test_the_consumer_stream_sees_the_pixels(torch):
    """decode(out=tensor) under a non-default stream that is busy -- the tensor comes from the caching allocator on that
    stream, behind work that may still use its memory -- and a consumer kernel enqueued on the stream right after: it
    reads the decoded pixels, with no synchronisation in between."""
    import guetzli_amd
    w, h = 64, 48
    jpeg, _ = guetzli_amd.process(images.crop(w, h, 90, 70))
    exp = guetzli_amd.decode(jpeg, device="host")
    busy = torch.ones((2048, 2048), device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(8):
            busy = busy @ busy * 0.0 + 1.0
        out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        guetzli_amd.decode(jpeg, out=out)
        total = out.to(torch.int64).sum()      # the consumer, on s
        copy = out.clone()
    torch.cuda.synchronize()
    assert int(total) == int(exp.astype(np.int64).sum())
    assert np.array_equal(copy.cpu().numpy(), exp)


# ------------------------------------------------------------------ process(decoded=) ----
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


def test_bees_decoded_is_the_reconstruction_of_the_output(torch, L):
    import guetzli_amd
    bees = images.bees()
    jpeg, info = guetzli_amd.process(torch.from_numpy(bees).cuda(), decoded=True)
    assert sha(jpeg) == BEES_Q95_SHA   # nothing about the encode moved
    t = info["decoded"]
    assert t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (258, 444, 3)
    co, factor = coefficients_of(jpeg)
    assert factor == 1
    with L.context(bees, TARGET) as ctx:
        ctx.set_coeffs(co)
        exp = ctx.reconstruct()[0]
    assert np.array_equal(t.cpu().numpy(), exp)
    assert info["timers"]["decode_output"] > 0


def test_process_many_decoded(torch):
    import guetzli_amd
    batch = np.stack([images.crop(64, 64, 40 * k, 30 * k) for k in range(4)])
    many = guetzli_amd.process_many(torch.from_numpy(batch).cuda(), workers=4, decoded=True)
    assert [m[0] for m in many] == [guetzli_amd.process(batch[k])[0] for k in range(4)]
    for jpeg, info in many:
        assert np.array_equal(info["decoded"].cpu().numpy(), guetzli_amd.decode(jpeg, device="host"))


def test_small_and_host_inputs_are_decoded_too(torch):
    """An image too small for a context, and host pixels: the decode is of the returned bytes, whatever path wrote them."""
    import guetzli_amd
    for w, h in ((16, 16), (40, 33)):
        jpeg, info = guetzli_amd.process(images.crop(w, h, 100, 60), decoded=True)
        assert np.array_equal(info["decoded"].cpu().numpy(), guetzli_amd.decode(jpeg, device="host"))


# ------------------------------------------------------------------ refusals ----
def test_a_tensor_on_another_device_is_refused(torch, small_jpeg):
    import guetzli_amd
    t = torch.zeros((43, 61, 3), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(ValueError, match="device"):
        guetzli_amd.decode(small_jpeg[0], out=t, device=1)
    with pytest.raises(ValueError, match="share an address"):
        guetzli_amd.decode(small_jpeg[0], out=torch.zeros((43, 61, 1), dtype=torch.uint8, device="cuda").expand(43, 61, 3))
    with pytest.raises(ValueError, match="negative strides|shape"):
        guetzli_amd.decode(small_jpeg[0], out=torch.zeros((43, 61), dtype=torch.uint8, device="cuda"))


def test_a_host_pointer_is_an_argument_error_not_a_fault(torch, L):
    """Ordinary host memory where device memory is expected: GZ_E_ARG (by the return code alone), and the library goes
    on working."""
    from guetzli_amd.capi import GZ_DT_U8, device_output
    w, h = 64, 48
    co = doc.random_coeffs(w, h, 1, seed=5)
    buf = np.zeros((h, w, 3), np.uint8)
    o = device_output(buf.ctypes.data, GZ_DT_U8, (3 * w, 3, 1))
    assert L.lib.gz_decode_coeffs_device(0, co.ctypes.data, w, h, 1, C.byref(o)) == -1
    assert not buf.any()
    with L.context(images.crop(w, h), TARGET) as ctx:
        ctx.encode_rgb()
        ctx.quantize(None)
        assert L.lib.gz_reconstruct_device(ctx.handle, C.byref(o)) == -1
        exp = ctx.reconstruct()[0]
        d = OnDevice(torch, doc.destination(w, h, "uint8", "HWC"))
        ctx.reconstruct_device(d.output())
        d.check(exp)
