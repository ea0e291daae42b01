"""Device-resident pixels with alpha and 16-bit samples (gz_device_pixels: gz_create_from_device_pixels /
gz_set_rgb_device_pixels / gz_pack_rgb_device_pixels, gzh_process_device_pixels, guetzli_amd.process(...,
background=)) without a GPU: the kernels k_ingest_rgba and k_ingest_rgb<uint16> and their launch code through the CPU
emulation, where "device memory" is host memory; the argument checks of the PRODUCT library, which come before any
device call; the Python dispatch.  The rule they are held to is tests/device_alpha_cases.py's.  CPU only."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(HERE, "emu"), ROOT]
import build_emu  # noqa: E402
import device_alpha_cases as dac  # noqa: E402
import device_input_cases as dic  # noqa: E402
import fields  # noqa: E402
import images  # noqa: E402
from guetzli_amd import capi  # noqa: E402
from guetzli_amd.capi import Library, device_image, device_pixels  # noqa: E402
from guetzli_amd.encoder import DTYPE_CODES  # noqa: E402

TARGET = 0.971769
Q5 = np.full((3, 64), 5, np.int32)


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


def pixels_of(src, bg=(0, 0, 0), stream=0):
    """The gz_device_pixels of a dac.Source (or, opaque, of a dic.Source) whose buffers are host memory."""
    ptr = src.storage.ctypes.data + src.offset * src.itemsize
    alpha = 0
    if getattr(src, "alpha_storage", None) is not None:
        alpha = src.alpha_storage.ctypes.data + src.alpha_offset * src.itemsize
    return device_pixels(ptr, DTYPE_CODES[src.dtype], src.strides, stream, alpha, bg)


def pack(L, src, bg=(0, 0, 0)):
    return L.pack_rgb_device(pixels_of(src, bg), src.w, src.h)


# ------------------------------------------------------------------ pack parity ----
@pytest.mark.parametrize("layout", dac.LAYOUTS)
@pytest.mark.parametrize("dtype", dac.DTYPES)
def test_pack_parity(L, dtype, layout):
    """gz_pack_rgb_device_pixels against the numpy rule: widths 1, 3, 4, 5, 15, 16, 17, 33, 61, 64, 67 x heights 1, 2, 9,
    a random background each."""
    for src, bg in dac.parity_sources(dtype, layout):
        got = pack(L, src, bg)
        exp = src.expected(bg)
        assert np.array_equal(got, exp), (dtype, layout, src.w, src.h, bg, np.argwhere(got != exp)[:4])


@pytest.mark.parametrize("layout", dic.LAYOUTS)
def test_pack_parity_opaque_uint16(L, layout):
    """uint16 without alpha (k_ingest_rgb<uint16>): the high byte, whatever the background says."""
    rng = np.random.default_rng(5)
    for h in dac.HEIGHTS:
        for w in dac.WIDTHS:
            src = dac.lay_out_opaque(dac.random_storage("uint16", h * w * 3, rng).reshape(h, w, 3), "uint16", layout)
            got = pack(L, src, (9, 99, 199))
            exp = dac.expected_rgb(src.logical, None, "uint16")
            assert np.array_equal(got, exp), (layout, w, h)


@pytest.mark.parametrize("layout", ["HWC_rgba", "HWC_rgba_base1"])
def test_every_value_alpha_pair_under_every_background(L, layout):
    """All 65536 (v, a) pairs in every channel, through the four-vector path and element by element: the division is a
    floor of (v a + bg (255 - a) + 128) / 255, and every shortcut for it is off somewhere."""
    colour, alpha = dac.every_v_a_pair()
    src = dac.lay_out(colour, alpha, "uint8", layout)
    for bg in dac.EXHAUSTIVE_BACKGROUNDS:
        got = pack(L, src, bg)
        exp = src.expected(bg)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, (layout, bg, [(tuple(i), int(got[tuple(i)]), int(exp[tuple(i)])) for i in bad[:4]])
    on_black = pack(L, src)
    assert on_black[127, 1, 0] == 1, "v = 1, a = 127: the reference's (v * a + 128) / 255 is 1, a rounding of v a / 255 gives 0"
    assert np.array_equal(on_black[255], colour[255]) and not on_black[0].any()


def test_the_numpy_rule_against_its_shortcuts():
    """(of the restatement itself) The three familiar shortcuts each differ from the rule on 128 of the 65536 pairs."""
    colour, alpha = dac.every_v_a_pair()
    v, a = colour[..., 0].astype(np.int64), alpha.astype(np.int64)
    rule = dac.blend(v, a, 0).astype(np.int64)
    assert np.array_equal(rule, (v * a + 128) // 255)
    t, u = v * a, v * a + 128
    assert np.count_nonzero(rule != ((u + (u >> 8)) >> 8)) == 128                    # with u = v a + 128: a rounding
    assert np.count_nonzero(rule != np.rint(t / 255.0).astype(np.int64)) == 128
    assert np.count_nonzero(rule != np.rint(t.astype(np.float32) * np.float32(1 / 255)).astype(np.int64)) == 128


@pytest.mark.parametrize("layout", ["HWC_rgba", "CHW_rgba", "HWC_rgba_base1"])
def test_every_uint16_pattern_as_value_and_as_alpha(L, layout):
    colour, alpha = dac.every_u16_pattern()
    src = dac.lay_out(colour, alpha, "uint16", layout)
    for bg in ((0, 0, 0), (255, 1, 128)):
        got = pack(L, src, bg)
        assert np.array_equal(got, src.expected(bg)), (layout, bg)


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_a_float_alpha_goes_through_the_float_byte_rule(L, dtype):
    """NaN is transparent, as -1 and -inf are; 2 and +inf are opaque."""
    bits = {"float32": np.array([np.nan, -1.0, 2.0, np.inf, -np.inf, 0.5, 1.0, 0.0], np.float32),
            "float16": np.array([0x7E00, 0xBC00, 0x4000, 0x7C00, 0xFC00, 0x3800, 0x3C00, 0x0000], np.uint16),
            "bfloat16": np.array([0x7FC0, 0xBF80, 0x4000, 0x7F80, 0xFF80, 0x3F00, 0x3F80, 0x0000], np.uint16)}[dtype]
    rng = np.random.default_rng(3)
    h, w = 4, 32
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    colour = dic.from_bytes(rgb, dtype)
    alpha = np.resize(bits, h * w).reshape(h, w)
    bg = (10, 200, 77)
    for layout in ("HWC_rgba", "CHW_rgba", "CHW_rgba_base1"):
        src = dac.lay_out(colour, alpha, dtype, layout)
        got = pack(L, src, bg)
        assert np.array_equal(got, src.expected(bg)), (dtype, layout)
        for k, opaque in enumerate((False, False, True, True, False)):
            assert np.array_equal(got[0, k], rgb[0, k] if opaque else np.array(bg, np.uint8)), (dtype, layout, k)


def test_the_fixtures_samples_pack_to_the_reference_pixels(L):
    """The raw samples of the three PNG fixtures through gz_pack_rgb_device_pixels hash to each fixture's rgb_sha256: the
    pixels the unmodified reference's ReadPNG made of the file."""
    for name, (samples, dtype) in dac.fixture_samples().items():
        h, w, ch = samples.shape
        ptr = samples.ctypes.data
        alpha = ptr + (ch - 1) * samples.itemsize if ch in (2, 4) else 0
        image = device_pixels(ptr, DTYPE_CODES[dtype], (w * ch, ch, 0 if ch == 2 else 1), 0, alpha)
        got = L.pack_rgb_device(image, w, h)
        assert hashlib.sha256(got.tobytes()).hexdigest() == dac.fixture(name)["rgb_sha256"], name


# ------------------------------------------------------------------ context parity ----
def rgba_case(w, h, x0, y0, seed):
    """(rgb bytes, alpha bytes, background, the host-blended bytes)."""
    rng = np.random.default_rng(seed)
    rgb = images.crop(w, h, x0, y0)
    alpha = rng.integers(0, 256, (h, w), dtype=np.uint8)
    alpha[::3, ::2] = 255
    alpha[1::4, 1::5] = 0
    bg = (30, 144, 255)
    return rgb, alpha, bg, dac.blend(rgb, alpha[..., None], bg)


def sources_of(rgb, alpha):
    """The bytes themselves as HWC RGBA, and k / 255 as float32 CHW RGBA."""
    return [dac.lay_out(rgb, alpha, "uint8", "HWC_rgba"),
            dac.lay_out(dic.from_bytes(rgb, "float32"), dic.from_bytes(alpha, "float32"), "float32", "CHW_rgba")]


def evaluate(ctx):
    co = ctx.encode_rgb()
    cq = ctx.quantize(Q5)
    dist, dm, bm = ctx.compare()
    return co, cq, np.float32(dist), dm, bm


def assert_same_evaluation(a, b):
    for x, y, what in zip(a, b, ("gz_encode_rgb coefficients", "quantised coefficients", "distance", "distance map", "block maxima")):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), what


@pytest.mark.parametrize("w,h", [(61, 43), (33, 32)])
def test_context_from_rgba_pixels_equals_context_from_the_blended_bytes(L, w, h):
    rgb, alpha, bg, blended = rgba_case(w, h, 50, 40, 1)
    with L.context(blended, TARGET) as ctx:
        exp = evaluate(ctx)
    for src in sources_of(rgb, alpha):
        assert np.array_equal(src.expected(bg), blended)
        with L.context_from_device(pixels_of(src, bg), w, h, TARGET) as ctx:
            assert_same_evaluation(evaluate(ctx), exp)


def test_set_rgb_device_pixels_on_a_used_context(L):
    w, h = 61, 43
    first = images.crop(w, h, 0, 0)
    rgb, alpha, bg, blended = rgba_case(w, h, 120, 90, 2)
    with L.context(blended, TARGET) as ctx:
        exp = evaluate(ctx)
    for src in sources_of(rgb, alpha):
        with L.context(first, TARGET) as ctx:
            evaluate(ctx)
            ctx.set_rgb_device(pixels_of(src, bg))
            assert_same_evaluation(evaluate(ctx), exp)


# ------------------------------------------------------------------ whole encodes ----
@pytest.mark.parametrize("w,h", [(40, 33), (16, 16)])
def test_process_device_pixels_gives_the_bytes_of_process_of_the_blended_bytes(host, w, h):
    """gzh_process_device_pixels through a context (40 x 33) and, too small for one (16 x 16), through
    gz_pack_rgb_device_pixels and the unquantised JPEG."""
    rgb, alpha, bg, blended = rgba_case(w, h, 100, 60, 3)
    exp, _ = host.process(blended, quality=95.0)
    assert exp != host.process(rgb, quality=95.0)[0]
    u16 = dac.lay_out((rgb.astype(np.uint16) << 8) | 0x5A, (alpha.astype(np.uint16) << 8) | 0xC3, "uint16", "CHW_rgba")
    for src in sources_of(rgb, alpha) + [u16]:
        assert src.alpha_storage is src.storage
        ptr = src.storage.ctypes.data + src.offset * src.itemsize
        got, info = host.process_device(ptr, w, h, src.dtype, src.strides, quality=95.0,
                                        alpha_offset=src.alpha_offset - src.offset, background=bg)
        assert got == exp, (src.dtype, len(got), len(exp))
        assert "timers" in info


# ------------------------------------------------------------------ enqueue order ----
GOLDEN = os.path.join(HERE, "golden", "enqueue_order")
W, H = 100, 84
PRODUCER = 0x5EED0   # a stream handle of the caller's: the emulation only names it


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


def life_of_a_context(L, image_of):
    """tests/test_device_input_emu.py's scenario: a context from a device image behind a producer stream, the original
    replaced without one, the context's end."""
    with Log(L) as log:
        with L.context_from_device(image_of(PRODUCER), W, H, TARGET) as ctx:
            ctx.set_rgb_device(image_of(0))
    return log.text.splitlines()


def test_enqueue_order_with_alpha_and_without(L):
    with open(os.path.join(GOLDEN, "create_from_device.txt")) as f:
        golden = f.read().splitlines()
    rgb = fields.primaries(W, H)
    opaque = dic.lay_out(rgb, "uint8", "HWC")
    # opaque pixels, through the old entries and through the new ones: the recorded order, line for line
    ptr = opaque.storage.ctypes.data
    assert life_of_a_context(L, lambda s: device_image(ptr, capi.GZ_DT_U8, opaque.strides, s)) == golden
    assert life_of_a_context(L, lambda s: pixels_of(opaque, stream=s)) == golden
    # pixels with alpha: one record / wait pair, ONE ingest launch of the same grid in k_ingest_rgb's place, the same tail
    src = dac.lay_out(rgb, np.full((H, W), 200, np.uint8), "uint8", "HWC_rgba")
    got = life_of_a_context(L, lambda s: pixels_of(src, (1, 2, 3), s))
    ingest = [i for i, ln in enumerate(golden) if ln.startswith("launch k_ingest_rgb ")]
    assert len(ingest) == 2 and ingest[0] == 2 and golden[0].startswith("record ") and golden[1].startswith("wait ")
    assert len(got) == len(golden)
    for i, (g, e) in enumerate(zip(got, golden)):
        assert g == (e.replace("launch k_ingest_rgb ", "launch k_ingest_rgba ") if i in ingest else e), (i, g, e)
    assert sum(ln.startswith(("record ", "wait ")) for ln in got) == 2
    assert sum(ln.startswith("launch k_ingest") for ln in got) == 2


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
    buf = np.zeros(64 * 64 * 4, np.uint8)
    out = np.zeros(64 * 64 * 3, np.uint8)
    good = dict(ptr=buf.ctypes.data, dtype=capi.GZ_DT_U8, strides=(256, 4, 1), alpha=buf.ctypes.data + 3)

    def img(**kw):
        a = dict(good, **kw)
        return device_pixels(a["ptr"], a["dtype"], a["strides"], 0, a["alpha"], (1, 2, 3))

    def create(image, w=64, h=64):
        err = C.c_int(0)
        ctx = lib.gz_create_from_device_pixels(0, w, h, C.byref(image) if image is not None else None, 1.0, C.byref(err))
        assert not ctx
        return err.value

    def pack_rc(image, w=64, h=64, dst=out):
        return lib.gz_pack_rgb_device_pixels(0, C.byref(image) if image is not None else None, w, h, dst.ctypes.data if dst is not None else None)

    wrong_size, old_size = img(), img()
    wrong_size.struct_size -= 8
    old_size.struct_size = C.sizeof(capi.GzDeviceImage)
    too_far = img(strides=(1 << 57, 4, 1))          # 63 rows of 2^57 elements: the last offset needs more than 62 bits
    alpha_too_far = img(strides=(1 << 56, 1 << 56, 0), alpha=buf.ctypes.data + 1)   # (h-1) sy + (w-1) sx alone: alpha's extent
    bad = [None, img(ptr=0), wrong_size, old_size, img(dtype=-1), img(dtype=5), img(strides=(-256, 4, 1)), img(strides=(256, -4, 1)),
           img(strides=(256, 4, -1)), too_far, alpha_too_far, img(strides=(0, 0, 1 << 61))]
    for image in bad:
        assert create(image) == -1
        assert pack_rc(image) == -1
        assert lib.gz_set_rgb_device_pixels(None, C.byref(image) if image is not None else None) == -1
    for w, h in ((7, 64), (64, 7), (1 << 16, 64), (64, 1 << 16), (0, 64)):    # gz_create's limits
        assert create(img(), w, h) == -1
    for w, h in ((0, 64), (64, 0), (1 << 16, 64), (64, 1 << 16), (-1, 64)):   # the pack's: 0 < w, h < 65536
        assert pack_rc(img(), w, h) == -1
    assert pack_rc(img(), dst=None) == -1
    if not has_gpu():   # valid arguments: the device is asked for, and there is none -- no fallback
        for image in (img(), img(alpha=0), img(dtype=capi.GZ_DT_U16), img(dtype=capi.GZ_DT_U16, alpha=0)):
            assert create(image) == -2
            assert pack_rc(image) == -2
            assert pack_rc(image, 3, 5) == -2
    # the older struct and its entries accept what they accepted: no GZ_DT_U16, no other struct
    old = device_image(buf.ctypes.data, capi.GZ_DT_U16, (192, 3, 1))
    err = C.c_int(0)
    assert not lib.gz_create_from_device(0, 64, 64, C.byref(old), 1.0, C.byref(err)) and err.value == -1
    assert lib.gz_pack_rgb_device(0, C.byref(old), 64, 64, out.ctypes.data) == -1
    assert lib.gz_set_rgb_device(None, C.byref(old)) == -1
    assert not lib.gz_create_from_device(0, 64, 64, C.byref(img()), 1.0, C.byref(err)) and err.value == -1
    assert lib.gz_pack_rgb_device(0, C.byref(img()), 64, 64, out.ctypes.data) == -1


# ------------------------------------------------------------------ the Python dispatch ----
from fake_device import FakeDeviceAddress as FakeDeviceArray  # noqa: E402


class StubHost:
    def __init__(self):
        self.calls = []

    def process(self, rgb, **kw):
        self.calls.append(("process", np.array(rgb), kw))
        return b"host", {}

    def process_device(self, ptr, w, h, dtype, strides, **kw):
        self.calls.append(("process_device", (ptr, w, h, dtype, tuple(strides)), kw))
        return b"device", {}


@pytest.fixture()
def stub(monkeypatch):
    from guetzli_amd import encoder
    s = StubHost()
    monkeypatch.setattr(encoder, "_default", s)
    return s


PTR = 0x7F0000000000


def test_dispatch_of_channel_counts(stub):
    import guetzli_amd
    cases = [((4, 20, 17), "|u1", 0, (PTR, 17, 20, "uint8", (17, 1, 340)), 1020, (0, 0, 0)),
             ((20, 17, 4), "|u1", (1, 2, 3), (PTR, 17, 20, "uint8", (68, 4, 1)), 3, (1, 2, 3)),
             ((2, 20, 17), "<f4", [255, 0, 7], (PTR, 17, 20, "float32", (17, 1, 0)), 340, (255, 0, 7)),
             ((20, 17, 2), "<u2", 128, (PTR, 17, 20, "uint16", (34, 2, 0)), 1, (128, 128, 128)),
             ((1, 20, 17), "|u1", None, (PTR, 17, 20, "uint8", (17, 1, 0)), None, None),
             ((20, 17, 1), "<f2", None, (PTR, 17, 20, "float16", (17, 1, 0)), None, None),
             ((20, 17, 3), "<u2", None, (PTR, 17, 20, "uint16", (51, 3, 1)), None, None),
             ((20, 17, 3), "|u1", (9, 9, 9), (PTR, 17, 20, "uint8", (51, 3, 1)), None, None),    # opaque: no effect
             ((20, 17), "<u2", 0, (PTR, 17, 20, "uint16", (17, 1, 0)), None, None)]
    for shape, typestr, background, placed, alpha, bg in cases:
        assert guetzli_amd.process(FakeDeviceArray(shape, typestr), quality=90, background=background)[0] == b"device"
        name, got, kw = stub.calls[-1]
        assert name == "process_device" and got == placed, shape
        assert kw.get("alpha_offset") == alpha and kw.get("background") == bg, (shape, kw)
        assert kw["quality"] == 90 and kw["stream"] == 0 and kw["device"] == 0


def test_nothing_is_blended_without_the_keyword(stub):
    import guetzli_amd
    for shape in ((20, 17, 4), (4, 20, 17), (20, 17, 2), (2, 20, 17)):
        with pytest.raises(ValueError, match="background="):
            guetzli_amd.process(FakeDeviceArray(shape))
        for layout in ("HWC", "CHW"):
            if shape[0 if layout == "CHW" else 2] in (2, 4):
                with pytest.raises(ValueError, match="background="):
                    guetzli_amd.process(FakeDeviceArray(shape), layout=layout)
    for bad in ((1, 2), (1, 2, 3, 4), 256, -1, (0, 0, 256), 1.5, (0.0, 0.0, 0.0), "white", True, [None] * 3):
        with pytest.raises(ValueError, match="background"):
            guetzli_amd.process(FakeDeviceArray((20, 17, 4)), background=bad)
        with pytest.raises(ValueError, match="background"):
            guetzli_amd.process(images.crop(40, 33), background=bad)
    with pytest.raises(ValueError):
        guetzli_amd.process(FakeDeviceArray((20, 17, 5)), background=0)
    with pytest.raises(ValueError):
        guetzli_amd.process(FakeDeviceArray((20, 17, 5)), background=0, layout="HWC")
    assert stub.calls == []


def test_layout_none_with_the_new_channel_counts(stub):
    import guetzli_amd

    def placed(shape, **kw):
        guetzli_amd.process(FakeDeviceArray(shape), **kw)
        return stub.calls[-1][1][1:3] + (stub.calls[-1][1][4],), stub.calls[-1][2].get("alpha_offset")

    # today's rule first: a 3 decides, whatever the other end is
    assert placed((1, 17, 3)) == ((17, 1, (51, 3, 1)), None)
    assert placed((1, 17, 3), background=0) == ((17, 1, (51, 3, 1)), None)
    assert placed((3, 17, 1)) == ((1, 17, (1, 1, 17)), None)
    assert placed((3, 17, 4), background=0) == ((4, 17, (4, 1, 68)), None)
    assert placed((4, 17, 3), background=0) == ((17, 4, (51, 3, 1)), None)
    with pytest.raises(ValueError, match="ambiguous"):
        placed((3, 17, 3), background=0)
    # no 3: a 1 -- or, with background=, a 1, 2 or 4 -- decides
    assert placed((1, 17, 4)) == ((4, 17, (4, 1, 0)), None)             # without the keyword 4 does not qualify
    assert placed((5, 17, 4), background=0) == ((17, 5, (68, 4, 1)), 3)
    assert placed((2, 17, 5), background=0) == ((5, 17, (5, 1, 0)), 85)
    for shape, kw in (((1, 17, 1), {}), ((1, 17, 4), dict(background=0)), ((4, 17, 4), dict(background=0)),
                      ((4, 17, 2), dict(background=0)), ((2, 17, 1), dict(background=0))):
        with pytest.raises(ValueError, match="ambiguous"):
            placed(shape, **kw)
    n = len(stub.calls)
    for shape, kw in (((5, 17, 6), {}), ((5, 17, 6), dict(background=0)), ((4, 17, 4), {}), ((2, 17, 5), {})):
        with pytest.raises(ValueError):
            placed(shape, **kw)
    assert len(stub.calls) == n
    # an explicit layout always decides
    assert placed((4, 17, 4), background=0, layout="HWC") == ((17, 4, (68, 4, 1)), 3)
    assert placed((4, 17, 4), background=0, layout="CHW") == ((4, 17, (4, 1, 68)), 204)
    assert placed((1, 17, 1), layout="CHW") == ((1, 17, (1, 1, 0)), None)


def test_process_many_passes_the_background_on(stub):
    import guetzli_amd
    out = guetzli_amd.process_many([FakeDeviceArray((20, 17, 4), "|u1", 0x5EED0 + k) for k in range(5)], workers=3,
                                   quality=90, background=(4, 5, 6))
    assert [o[0] for o in out] == [b"device"] * 5
    assert all(c[2]["background"] == (4, 5, 6) and c[2]["alpha_offset"] == 3 and c[2]["quality"] == 90 for c in stub.calls)
    assert sorted(c[2]["stream"] for c in stub.calls) == [0x5EED0 + k for k in range(5)]
    with pytest.raises(ValueError, match="background="):
        guetzli_amd.process_many([FakeDeviceArray((20, 17, 4))])


def test_host_arrays_are_blended_in_numpy_and_take_the_old_path(stub):
    import guetzli_amd
    rgb, alpha, bg, blended = rgba_case(40, 33, 10, 10, 4)
    rgba = np.concatenate([rgb, alpha[..., None]], -1)
    assert guetzli_amd.process(rgba, background=bg, quality=90.0)[0] == b"host"
    assert np.array_equal(stub.calls[-1][1], blended) and stub.calls[-1][2] == {"quality": 90.0, "device": 0}
    ga = np.ascontiguousarray(rgba[..., 1::2])
    assert guetzli_amd.process(ga, background=7)[0] == b"host"
    assert np.array_equal(stub.calls[-1][1], dac.blend(np.repeat(ga[..., :1], 3, -1), ga[..., 1:], 7))
    assert np.array_equal(guetzli_amd.blend_on_background(rgba, bg), blended)
    assert guetzli_amd.process(rgb, background=bg)[0] == b"host"      # opaque: no effect
    assert np.array_equal(stub.calls[-1][1], rgb)
    assert guetzli_amd.process_many([rgba, rgba], background=bg)[1][0] == b"host"
    assert np.array_equal(stub.calls[-1][1], blended)


# ------------------------------------------------------------------ bounds, under the host sanitizers ----
def test_alpha_ingest_reads_stay_inside_their_sources(tmp_path):
    """tests/cpp/ingest_alpha_bounds.cc: gz_pack_rgb_device_pixels on colour and alpha sources malloc'ed to exactly their
    last addressed element + 1, every layout x element type x width, built as a plain program with AddressSanitizer and
    UBSan (unoptimised: the whole emulated library is its one translation unit)."""
    exe = str(tmp_path / "ingest_alpha_bounds")
    subprocess.run(["g++", "-O0", "-std=c++17", "-ffp-contract=off", "-DGZ_EMU", "-DGZ_NO_PROBES", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-w", "-I" + os.path.join(ROOT, "tests", "emu"), "-x", "c++",
                    os.path.join(ROOT, "tests", "cpp", "ingest_alpha_bounds.cc"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "2706 cases, all bytes as expected" in out.stdout
