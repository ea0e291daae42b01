"""Device-resident output (gz_decode_coeffs_device / gz_decode_coeffs / gz_reconstruct_device, guetzli_amd::DecodeJpegToRGB,
guetzli_amd.decode and process(decoded=)) without a GPU: the kernel k_emit_rgb and the context-free decode through the CPU
emulation, where "device memory" is host memory and numpy buffers serve as destinations; the argument checks of the
PRODUCT library, which come before any device call; the Python surface.  CPU only."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(HERE, "emu")]
import build_emu  # noqa: E402
import device_input_cases as dic  # noqa: E402
import device_output_cases as doc  # noqa: E402
import images  # noqa: E402
from checkers import oracle, ref  # noqa: E402
from guetzli_amd import capi  # noqa: E402
from guetzli_amd.capi import Library, device_image, device_output, device_pixels  # noqa: E402
from guetzli_amd.encoder import DTYPE_CODES  # noqa: E402

needs_ref = pytest.mark.skipif(ref is None, reason="oracle/_ref/libgz_ref.so not built")
CHECKERS = [pytest.param(oracle, id="oracle"), pytest.param(ref, id="ref", marks=needs_ref)]
SIZES = [(1, 1), (7, 5), (8, 8), (17, 9), (33, 31), (61, 43)]
CONSUMER = 0x5EED0   # a stream handle of the caller's: the emulation only names it


@pytest.fixture(scope="module")
def L():
    lib = Library(build_emu.build())
    lib.lib.gz_emu_enqueue_log_fetch.restype = C.c_long
    lib.lib.gz_emu_enqueue_log_fetch.argtypes = [C.c_char_p, C.c_long]
    return lib


@pytest.fixture(scope="module")
def host():
    from guetzli_amd.encoder import HostLibrary
    return HostLibrary(build_emu.build_host())


def output_of(dest, stream=0):
    return device_output(dest.address, DTYPE_CODES[dest.dtype], dest.strides, stream)


def decode_into(L, co, w, h, dest, factor=1, stream=0):
    L.decode_coeffs_device(co, w, h, output_of(dest, stream), chroma_factor=factor)


# ------------------------------------------------------------------ the value rule ----
def test_the_rule_maps_every_byte_back():
    """(of the numpy restatement the other tests compare against) ingest_byte(emit(b)) == b for all 256 bytes in all five
    types; the float32 elements are the quotients, which b * (1 / 255.f) misses for 126 bytes; the bfloat16 rounding
    is torch's."""
    k = np.arange(256, dtype=np.uint8)
    for dtype in doc.DTYPES:
        e = doc.emitted(k, dtype)
        back = (e >> 8).astype(np.uint8) if dtype == "uint16" else dic.expected_bytes(e, dtype)
        assert np.array_equal(back, k), dtype
    f = doc.emitted(k, "float32")
    assert int((f != k.astype(np.float32) * (np.float32(1) / np.float32(255))).sum()) == 126
    import torch
    t = torch.from_numpy(f)
    assert np.array_equal(t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16), doc.emitted(k, "bfloat16"))
    assert np.array_equal(t.to(torch.float16).view(torch.int16).numpy().view(np.uint16), doc.emitted(k, "float16"))


# ------------------------------------------------------------------ emit parity, sentinels ----
@pytest.fixture(scope="module")
def decoded_cases(L):
    """Coefficients and their pixels (gz_decode_coeffs: checked against the reference below) for every width x height
    of the issue, computed once."""
    out = {}
    for h in doc.HEIGHTS:
        for w in doc.WIDTHS:
            co = doc.random_coeffs(w, h, 1, seed=1000 * h + w)
            out[(w, h)] = (co, L.decode_coeffs(co, w, h))
    assert np.array_equal(out[(67, 9)][1], oracle.reconstruct(out[(67, 9)][0], 67, 9)[1])
    return out


@pytest.mark.parametrize("layout", doc.LAYOUTS)
@pytest.mark.parametrize("dtype", doc.DTYPES)
def test_emit_parity_and_untouched_neighbours(L, decoded_cases, dtype, layout):
    """Every element of the image is the rule's, and every byte of the buffer outside the image's (y, x, c) set is the
    sentinel it was filled with: widths 1 .. 67 x heights 1, 2, 9."""
    for (w, h), (co, rgb) in decoded_cases.items():
        dest = doc.destination(w, h, dtype, layout)
        decode_into(L, co, w, h, dest)
        dest.check(rgb, what=layout)


@pytest.mark.parametrize("dtype", doc.DTYPES)
def test_all_256_bytes_round_trip_through_the_ingest_kernel(L, dtype):
    """A frame whose pixels take every byte value, decoded into `dtype` and read back by gz_pack_rgb_device: the bytes
    of gz_decode_coeffs again."""
    co, w, h = doc.all_bytes_coeffs(lambda c, ww, hh: oracle.reconstruct(c, ww, hh)[1])
    rgb = L.decode_coeffs(co, w, h)
    assert set(np.unique(rgb).tolist()) == set(range(256))
    for layout in ("HWC", "CHW", "HWC_base1"):
        dest = doc.destination(w, h, dtype, layout)
        decode_into(L, co, w, h, dest)
        dest.check(rgb)
        code = DTYPE_CODES[dtype]
        image = device_pixels(dest.address, code, dest.strides) if dtype == "uint16" else device_image(dest.address, code, dest.strides)
        assert np.array_equal(L.pack_rgb_device(image, w, h), rgb), (dtype, layout)


# ------------------------------------------------------------------ decode against the reference ----
def frames(w, h, factor):
    """Coefficients of a w x h frame: random ones, and (where the front end runs) those of a crop of bees.png."""
    yield "random", doc.random_coeffs(w, h, factor, seed=7 * w + h)
    co = oracle.encode_rgb(images.crop(w, h, 120, 80))
    if factor == 1:
        yield "bees", co
    elif w >= 8 and h >= 8:
        yield "bees", oracle.downsample(co, w, h)


@pytest.mark.parametrize("factor", [1, 2])
@pytest.mark.parametrize("chk", CHECKERS)
def test_decode_coeffs_is_to_srgb_of_the_reference(L, chk, factor):
    """gz_decode_coeffs and gz_decode_coeffs_device against OutputImage::ToSRGB, byte for byte, from 1 x 1 on."""
    for w, h in SIZES:
        for name, co in frames(w, h, factor):
            exp = (chk.reconstruct if factor == 1 else chk.reconstruct420)(co, w, h)[1]
            got = L.decode_coeffs(co, w, h, factor)
            assert np.array_equal(got, exp), (name, w, h, factor, np.argwhere(got != exp)[:4])
            dest = doc.destination(w, h, "uint8", "HWC")
            decode_into(L, co, w, h, dest, factor)
            dest.check(exp, what=name)


def test_reconstruct_device_is_reconstruct(L):
    """gz_reconstruct_device writes gz_reconstruct's srgb, in both frames, with and without a consumer stream."""
    w, h = 61, 43
    rgb = images.crop(w, h, 50, 40)
    q = np.full((3, 64), 5, np.int32)
    with L.context(rgb, 1.0) as ctx:
        ctx.encode_rgb()
        for frame in (1, 2):
            if frame == 2:
                ctx.downsample()
            ctx.quantize(q)
            exp = ctx.reconstruct()[0]
            for dtype, layout, stream in (("uint8", "HWC_crop", 0), ("bfloat16", "CHW", CONSUMER), ("float32", "WHC", 0)):
                dest = doc.destination(w, h, dtype, layout)
                ctx.reconstruct_device(output_of(dest, stream))
                ctx.synchronize()
                dest.check(exp, what=(frame, dtype, layout))
            assert np.array_equal(ctx.reconstruct()[0], exp)


# ------------------------------------------------------------------ JPEG streams ----
def jpeg_bytes(rgb, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", **kw)
    return b.getvalue()


def ref_decoded(data):
    """The reference's DecodeJpegToRGB by its parts: ReadJpeg's coefficients, dequantised as CopyFromJpegData does, and
    OutputImage::ToSRGB of them."""
    f = ref.lib.ref_read_jpeg
    f.restype, f.argtypes = C.c_long, [C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    buf = np.frombuffer(data, np.uint8)
    out = np.zeros(1 << 24, np.uint8)
    n = f(buf.ctypes.data, len(data), out.ctypes.data, out.size)
    assert 0 < n <= out.size
    j = doc.parse_jpeg_dump(out[:n].tobytes())
    co, factor = doc.frame_of_dump(j)
    return (ref.reconstruct if factor == 1 else ref.reconstruct420)(co, j["w"], j["h"])[1], len(j["components"]), factor


def jpeg_streams(host):
    """(name, bytes, components, chroma factor) of the streams of the issue."""
    q = np.stack([np.full(64, 3), np.full(64, 5), np.full(64, 7)]).astype(np.int32)
    q[:, 0] = 2
    for w, h, factor in ((40, 33, 1), (61, 43, 2), (17, 9, 1), (8, 8, 2)):
        co = doc.random_coeffs(w, h, factor, seed=w + h)
        nb, nbc = doc.blocks(w, h, factor)
        comp = np.repeat(np.arange(3), [nb, nbc, nbc])
        flat = co.reshape(-1, 64).astype(np.int32)
        flat = (flat // q[comp]) * q[comp]                       # multiples of the quantiser: what a JPEG can hold
        coq = flat.astype(np.int16).reshape(co.shape)
        yield f"host writer {w}x{h} factor {factor}", host.write_jpeg(coq, w, h, q, factor), 3, factor
        writer = ref.write_jpeg if factor == 1 else ref.write_jpeg420
        yield f"reference writer {w}x{h} factor {factor}", writer(coq, w, h, q), 3, factor
    yield "reference Process 40x40", ref.process(images.crop(40, 40, 30, 30), 1.0)[0], 3, 1
    yield "reference Process 16x16", ref.process(images.crop(16, 16, 30, 30), 1.0)[0], 3, 1
    grey = np.repeat(images.crop(40, 36, 10, 10)[:, :, 1:2], 3, axis=2)
    yield "reference Process of grey pixels", ref.process(grey, 1.0)[0], 1, 1
    yield "a one-component file 33x31", jpeg_bytes(np.ascontiguousarray(images.crop(33, 31)[:, :, 1]), quality=90), 1, 1
    yield "a 4:2:0 file 61x43", jpeg_bytes(images.crop(61, 43), quality=85, subsampling=2), 3, 2
    yield "a progressive 4:4:4 file", jpeg_bytes(images.crop(48, 40), quality=92, subsampling=0, progressive=True), 3, 1


@needs_ref
def test_decode_of_jpeg_streams(host):
    """guetzli_amd::DecodeJpegToRGB, to the host and into a device image, against the reference's reader, dequantisation
    and ToSRGB: the host writer's and the reference's streams, a one-component file, 4:2:0 off the MCU grid."""
    seen = set()
    for name, data, ncomp, factor in jpeg_streams(host):
        exp, ncomp_ref, factor_ref = ref_decoded(data)
        assert (ncomp_ref, factor_ref) == (ncomp, factor), name
        seen.add((ncomp, factor))
        h, w, _ = exp.shape
        assert host.jpeg_size(data) == (w, h), name
        got = host.decode_jpeg(data)
        assert np.array_equal(got, exp), (name, np.argwhere(got != exp)[:4])
        for dtype, layout in (("uint8", "HWC"), ("float16", "CHW_crop")):
            dest = doc.destination(w, h, dtype, layout)
            host.decode_jpeg_device(data, dest.address, dtype, dest.strides)
            dest.check(exp, what=name)
    assert seen == {(3, 1), (3, 2), (1, 1)}


def without_jfif_as_rgb(data):
    """A three-component baseline stream without its APP0 segment and with the component ids 'R', 'G', 'B': what
    libjpeg -- and the reference -- take for RGB, not YCbCr."""
    i = data.index(b"\xff\xe0")
    n = (data[i + 2] << 8) | data[i + 3]
    d = bytearray(data[:i] + data[i + 2 + n:])
    sof = d.index(b"\xff\xc0")
    sos = d.index(b"\xff\xda")
    for k, cid in enumerate(b"RGB"):
        d[sof + 10 + 3 * k] = cid
        d[sos + 5 + 2 * k] = cid
    return bytes(d)


def with_16_bit_quantisers(data):
    """The stream with its first quantisation table replaced by a 16-bit one of 65535s: every coefficient of that
    component that is not zero leaves int16 when it is dequantised."""
    i = data.index(b"\xff\xdb")
    n = (data[i + 2] << 8) | data[i + 3]
    assert n == 67 and data[i + 4] >> 4 == 0          # one 8-bit table in the segment
    return data[:i] + b"\xff\xdb" + bytes([0, 131, 0x10 | (data[i + 4] & 15)]) + b"\xff" * 128 + data[i + 2 + n:]


def test_streams_that_are_refused(host, capfd):
    good = jpeg_bytes(images.crop(48, 40), quality=90, subsampling=0)
    assert host.decode_jpeg(good).shape == (40, 48, 3)
    dest = doc.destination(48, 40, "uint8", "HWC")
    rgb_ids = without_jfif_as_rgb(good)
    assert host.jpeg_size(rgb_ids) == (48, 40)           # readable, but not YCbCr
    s422 = jpeg_bytes(images.crop(48, 40), quality=90, subsampling=1)
    for bad in (rgb_ids, s422):
        with pytest.raises(ValueError):
            host.decode_jpeg(bad)
        with pytest.raises(RuntimeError):
            host.decode_jpeg_device(bad, dest.address, "uint8", dest.strides)
    assert "Unsupported input JPEG" in capfd.readouterr().err
    big = with_16_bit_quantisers(good)
    assert host.jpeg_size(big) == (48, 40)               # readable, but the coefficients do not fit the frame's int16
    with pytest.raises(ValueError):
        host.decode_jpeg(big)
    assert "unexpectedly large coefficient values" in capfd.readouterr().err
    for bad in (good[: len(good) // 2], good[:2], b""):
        with pytest.raises(ValueError):
            host.decode_jpeg(bad)
        with pytest.raises(RuntimeError):
            host.decode_jpeg_device(bad, dest.address, "uint8", dest.strides)
    with pytest.raises(RuntimeError):                     # a destination made for another size is not written
        host.decode_jpeg_device(good, dest.address, "uint8", dest.strides, size=(40, 48))
    assert "the destination was made for 40 x 48" in capfd.readouterr().err
    assert np.array_equal(dest.raw, dest.before)          # nothing was written


# ------------------------------------------------------------------ enqueue order ----
class Log:
    def __init__(self, L):
        self.lib = L.lib

    def __enter__(self):
        self.lib.gz_emu_enqueue_log_start()
        return self

    def __exit__(self, *a):
        self.lib.gz_emu_enqueue_log_stop()
        n = self.lib.gz_emu_enqueue_log_fetch(None, 0)
        buf = C.create_string_buffer(n + 1)
        self.lib.gz_emu_enqueue_log_fetch(buf, n)
        self.text = buf.raw[:n].decode()


def test_the_stream_contract_in_both_directions(L):
    """With a consumer stream: its event is recorded and waited for before anything touches the destination, and it
    waits for an event recorded behind the emit kernel.  Without: no event at all, and the call synchronises."""
    w, h = 33, 9
    co = doc.random_coeffs(w, h, 2, seed=3)
    with Log(L) as log:
        decode_into(L, co, w, h, doc.destination(w, h, "float16", "CHW"), factor=2, stream=CONSUMER)
    lines = log.text.splitlines()
    kinds = [ln.split()[0] + (" " + ln.split()[1] if ln.startswith("launch") else "") for ln in lines]
    emit = [i for i, k in enumerate(kinds) if k.startswith("launch k_emit_rgb")]
    recon = [i for i, k in enumerate(kinds) if k.startswith("launch k_reconstruct420")]
    chroma = [i for i, k in enumerate(kinds) if k.startswith("launch k_chroma_samples")]
    assert len(emit) == len(recon) == len(chroma) == 1 and chroma[0] < recon[0] < emit[0]
    rec = [i for i, k in enumerate(kinds) if k == "record"]
    wait = [i for i, k in enumerate(kinds) if k == "wait"]
    assert len(rec) == len(wait) == 2
    assert rec[0] < wait[0] < chroma[0] and emit[0] < rec[1] < wait[1]
    lib_stream = lines[emit[0]].split()[-1]
    consumer = lines[rec[0]].split()[-1]
    assert consumer != lib_stream
    assert lines[wait[0]].split()[1] == lib_stream and lines[rec[1]].split()[-1] == lib_stream
    assert lines[wait[1]].split()[1] == consumer
    assert any(k == "stream_sync" for k in kinds[wait[1]:])
    with Log(L) as log:
        decode_into(L, co, w, h, doc.destination(w, h, "float16", "CHW"), factor=2)
    kinds = [ln.split()[0] for ln in log.text.splitlines()]
    assert "record" not in kinds and "wait" not in kinds and kinds[-1] == "stream_sync"


# ------------------------------------------------------------------ the product library's argument checks ----
@pytest.fixture(scope="module")
def product():
    from guetzli_amd import build as gzbuild
    return Library(gzbuild.build())


def has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_argument_errors_come_before_any_device_call(product):
    lib = product.lib
    assert lib.gz_abi_version() == 6
    w, h = 64, 48
    buf = np.zeros(w * h * 3 * 4, np.uint8)
    co = np.zeros((3, 48, 64), np.int16)
    good = dict(ptr=buf.ctypes.data, dtype=capi.GZ_DT_U8, strides=(3 * w, 3, 1))

    def out(**kw):
        a = dict(good, **kw)
        return device_output(a["ptr"], a["dtype"], a["strides"])

    def rc(o, w=w, h=h, factor=1, coeffs=co):
        return lib.gz_decode_coeffs_device(0, coeffs.ctypes.data if coeffs is not None else None, w, h, factor,
                                           C.byref(o) if o is not None else None)

    wrong_size = out()
    wrong_size.struct_size -= 8
    bad = [None, out(ptr=0), wrong_size, out(dtype=-1), out(dtype=5), out(strides=(-3 * w, 3, 1)), out(strides=(3 * w, -3, 1)),
           out(strides=(3 * w, 3, -1)), out(strides=(1 << 57, 3, 1)),              # the last offset needs more than 62 bits
           out(strides=(3 * w, 3, 0)), out(strides=(0, 3, 1)), out(strides=(3 * w, 0, 1)),   # a stride of 0
           out(strides=(3 * w - 1, 3, 1)),                                         # rows that overlap by one element
           out(strides=(3 * w, 2, 1)),                                             # pixels that overlap
           out(strides=(w, 1, w * h - 1)),                                         # planes that overlap
           out(strides=(1, 1, 1))]
    for o in bad:
        assert rc(o) == -1
        assert lib.gz_reconstruct_device(None, C.byref(o) if o is not None else None) == -1
    for o in (out(), out(strides=(w, 1, w * h)), out(strides=(3, 3 * h, 1)), out(strides=(4 * w, 4, 1)), out(dtype=capi.GZ_DT_U16)):
        assert lib.gz_reconstruct_device(None, C.byref(o)) == -1   # (no context)
    for ww, hh in ((0, 48), (64, 0), (1 << 16, 48), (64, 1 << 16), (-1, 48)):
        assert rc(out(), ww, hh) == -1
        assert lib.gz_decode_coeffs(0, co.ctypes.data, ww, hh, 1, buf.ctypes.data) == -1
    assert rc(out(), factor=0) == -1 and rc(out(), factor=3) == -1 and rc(out(), coeffs=None) == -1
    assert lib.gz_decode_coeffs(0, None, w, h, 1, buf.ctypes.data) == -1
    assert lib.gz_decode_coeffs(0, co.ctypes.data, w, h, 1, None) == -1
    if not has_gpu():   # valid arguments: the device is asked for, and there is none -- no fallback
        for o in (out(), out(strides=(w, 1, w * h)), out(strides=(3, 3 * h, 1)), out(strides=(4 * w, 4, 1))):
            assert rc(o) == -2
        assert rc(out(strides=(0, 3, 1)), h=1) == -2    # a dimension of one element: its stride does not count
        assert lib.gz_decode_coeffs(0, co.ctypes.data, w, h, 2, buf.ctypes.data) == -2
        assert lib.gz_decode_coeffs(0, co.ctypes.data, 1, 1, 1, buf.ctypes.data) == -2


# ------------------------------------------------------------------ the Python surface ----
import fake_device  # noqa: E402
from fake_device import FakeDeviceArray  # noqa: E402


@pytest.fixture()
def emulated(monkeypatch, host):
    """guetzli_amd's module-level functions on the emulated libraries, with numpy memory for the tensors they allocate."""
    from guetzli_amd import encoder
    monkeypatch.setattr(encoder, "_default", host)
    fake_device.install(monkeypatch)


@pytest.mark.parametrize("w,h", [(40, 40), (16, 16)])
def test_process_decoded_is_the_decode_of_the_returned_bytes(emulated, w, h):
    """process(decoded=True): through a context (40 x 40) and for an image too small for one (16 x 16)."""
    import guetzli_amd
    rgb = images.crop(w, h, 100, 60)
    exp_jpeg, _ = guetzli_amd.process(rgb)
    jpeg, info = guetzli_amd.process(rgb, decoded=True)
    assert jpeg == exp_jpeg
    exp = guetzli_amd.decode(jpeg, device="host")
    assert exp.shape == (h, w, 3) and exp.dtype == np.uint8
    assert np.array_equal(info["decoded"].array, exp)
    assert info["timers"]["decode_output"] > 0
    if w < 32:   # into a destination of the caller's: float32 CHW
        mine = FakeDeviceArray(np.zeros((3, h, w), np.float32))
        jpeg2, info2 = guetzli_amd.process(rgb, decoded=mine)
        assert jpeg2 == exp_jpeg and info2["decoded"] is mine
        assert np.array_equal(mine.array, doc.emitted(exp, "float32").transpose(2, 0, 1))


def test_decode_allocates_or_fills(emulated):
    import guetzli_amd
    rgb = images.crop(40, 33, 20, 20)
    jpeg, _ = guetzli_amd.process(rgb)
    exp = guetzli_amd.decode(jpeg, device="host")
    got = guetzli_amd.decode(jpeg, device=0)
    assert np.array_equal(got.array, exp)
    got = guetzli_amd.decode(jpeg, dtype="float16", layout="CHW", device=0)
    assert got.array.shape == (3, 33, 40) and np.array_equal(got.array.view(np.uint16), doc.emitted(exp, "float16").transpose(2, 0, 1))
    canvas = np.full((50, 60, 3), 7, np.uint8)
    view = canvas[5:38, 10:50]
    out = FakeDeviceArray(view, strides=view.strides)
    assert guetzli_amd.decode(jpeg, out=out) is out
    assert np.array_equal(view, exp)
    canvas[5:38, 10:50] = 7
    assert (canvas == 7).all()


def test_decode_refuses_what_it_cannot_fill(emulated):
    import guetzli_amd
    jpeg, _ = guetzli_amd.process(images.crop(40, 33, 20, 20))
    a = np.zeros((33, 40, 3), np.uint8)
    with pytest.raises(ValueError, match="negative strides"):
        guetzli_amd.decode(jpeg, out=FakeDeviceArray(a, strides=(120, -3, 1)))
    with pytest.raises(ValueError, match="share an address"):
        guetzli_amd.decode(jpeg, out=FakeDeviceArray(a, strides=(120, 3, 0)))
    with pytest.raises(ValueError, match="share an address"):
        guetzli_amd.decode(jpeg, out=FakeDeviceArray(a, strides=(119, 3, 1)))
    with pytest.raises(ValueError, match="read-only"):
        guetzli_amd.decode(jpeg, out=FakeDeviceArray(a, readonly=True))
    with pytest.raises(ValueError, match="shape"):
        guetzli_amd.decode(jpeg, out=FakeDeviceArray(np.zeros((40, 33, 3), np.uint8)))
    with pytest.raises(ValueError, match="shape"):
        guetzli_amd.decode(jpeg, out=FakeDeviceArray(a), layout="CHW")
    with pytest.raises(TypeError):
        guetzli_amd.decode(jpeg, out=FakeDeviceArray(np.zeros((33, 40, 3), np.int32)))
    with pytest.raises(ValueError, match="layout"):
        guetzli_amd.decode(jpeg, out=FakeDeviceArray(a), layout="WHC")
    with pytest.raises(ValueError):
        guetzli_amd.decode(jpeg, out=FakeDeviceArray(a), device="host")
    assert not a.any()
    with pytest.raises(ValueError, match="decoded"):
        guetzli_amd.process_many([images.crop(40, 33)], decoded=FakeDeviceArray(a))


# ------------------------------------------------------------------ bounds, under the host sanitizers ----
def test_emit_stores_stay_inside_the_destination(tmp_path):
    """tests/cpp/emit_bounds.cc: gz_decode_coeffs_device into destinations malloc'ed to exactly the last addressed element
    + 1, every layout x element type x size, built as a plain program with AddressSanitizer and UBSan (unoptimised: the
    whole emulated library is its one translation unit)."""
    import subprocess
    exe = str(tmp_path / "emit_bounds")
    subprocess.run(["g++", "-O0", "-std=c++17", "-ffp-contract=off", "-DGZ_EMU", "-DGZ_NO_PROBES", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-w", "-I" + os.path.join(ROOT, "tests", "emu"), "-x", "c++",
                    os.path.join(ROOT, "tests", "cpp", "emit_bounds.cc"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "1155 cases, all elements as expected, no store outside the destination" in out.stdout
