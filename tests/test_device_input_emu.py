"""Device-resident input (gz_create_from_device / gz_set_rgb_device / gz_pack_rgb_device, guetzli_amd::Process of a
DeviceImage, guetzli_amd.process of a GPU tensor) without a GPU: the kernel k_ingest_rgb and its launch code through
the CPU emulation, where "device memory" is host memory and numpy arrays serve as sources; the argument checks of the
PRODUCT library, which come before any device call; the Python dispatch.  CPU only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(HERE, "emu"), ROOT]   # (the second: run as a script, to record)
import build_emu  # noqa: E402
import device_input_cases as dic  # noqa: E402
import fields  # noqa: E402
import images  # noqa: E402
from guetzli_amd import capi  # noqa: E402
from guetzli_amd.capi import Library, device_image  # noqa: E402
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


def image_of(src, stream=0):
    """The gz_device_image of a dic.Source whose buffer is host memory."""
    ptr = src.storage.ctypes.data + src.offset * src.itemsize
    return device_image(ptr, DTYPE_CODES[src.dtype], src.strides, stream)


def pack(L, src):
    return L.pack_rgb_device(image_of(src), src.w, src.h)


# ------------------------------------------------------------------ pack parity ----
@pytest.mark.parametrize("layout", dic.LAYOUTS)
@pytest.mark.parametrize("dtype", dic.DTYPES)
def test_pack_parity(L, dtype, layout):
    """gz_pack_rgb_device against the numpy rule: widths 1, 3, 4, 5, 33, 61, 64, 67 x heights 1, 2, 9."""
    for src in dic.parity_sources(dtype, layout):
        got = pack(L, src)
        exp = dic.expected_bytes(src.logical, dtype)
        assert np.array_equal(got, exp), (dtype, layout, src.w, src.h, np.argwhere(got != exp)[:4])


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_pack_parity_exhaustive_floats(L, dtype):
    """Every float16 and every bfloat16 bit pattern; for float32 +-0, denormals, NaN, +-inf, +-1e30, 1, nextafter(1, 2),
    both sides of every tie (k + 0.5) / 255 and the ties themselves, random bit patterns."""
    for src in dic.exhaustive_sources(dtype):
        got = pack(L, src)
        exp = dic.expected_bytes(src.logical, dtype)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, (dtype, src.strides, [(tuple(i), hex(int(src.logical[tuple(i)].view(dic.STORAGE[dtype]
                                                                      if dtype != "float32" else np.uint32)))) for i in bad[:4]])


def test_the_rule_maps_k_over_255_back_to_k():
    """(of the numpy restatement the other tests compare against) k / 255 stored as float32, float16 or bfloat16 -> k."""
    k = np.arange(256, dtype=np.uint8)
    for dtype in ("float32", "float16", "bfloat16"):
        assert np.array_equal(dic.expected_bytes(dic.from_bytes(k, dtype), dtype), k)


# ------------------------------------------------------------------ context parity ----
def sources_of(rgb):
    """The two forms of the issue: the bytes themselves as HWC, and k / 255 as float32 CHW."""
    return [dic.lay_out(dic.from_bytes(rgb, "uint8"), "uint8", "HWC"), dic.lay_out(dic.from_bytes(rgb, "float32"), "float32", "CHW")]


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
def test_context_from_device_equals_context_from_host(L, w, h):
    rgb = images.crop(w, h, 50, 40)
    with L.context(rgb, TARGET) as ctx:
        exp = evaluate(ctx)
    for src in sources_of(rgb):
        with L.context_from_device(image_of(src), w, h, TARGET) as ctx:
            assert_same_evaluation(evaluate(ctx), exp)


def test_set_rgb_device_replaces_the_original_and_drops_the_stale_claims(L):
    """After a candidate and a Compare on other pixels (lin_is_cand, have_distmap, ... set), gz_set_rgb_device must leave
    the context as a fresh one on the new pixels is."""
    w, h = 61, 43
    first, second = images.crop(w, h, 0, 0), images.crop(w, h, 120, 90)
    with L.context(second, TARGET) as ctx:
        exp = evaluate(ctx)
    for src in sources_of(second):
        with L.context(first, TARGET) as ctx:
            evaluate(ctx)
            ctx.set_rgb_device(image_of(src))
            assert_same_evaluation(evaluate(ctx), exp)


# ------------------------------------------------------------------ whole encodes ----
@pytest.mark.parametrize("w,h", [(40, 33), (16, 16)])
def test_process_device_gives_the_bytes_of_process(host, w, h):
    """guetzli_amd::Process of a DeviceImage == Process of the same pixels from the host: through a context (40 x 33) and,
    for an image too small for one (16 x 16), through gz_pack_rgb_device and the unquantised JPEG."""
    rgb = images.crop(w, h, 100, 60)
    exp, _ = host.process(rgb, quality=95.0)
    for src in (dic.lay_out(dic.from_bytes(rgb, "uint8"), "uint8", "HWC"), dic.lay_out(dic.from_bytes(rgb, "float16"), "float16", "CHW")):
        ptr = src.storage.ctypes.data + src.offset * src.itemsize
        got, info = host.process_device(ptr, w, h, src.dtype, src.strides, quality=95.0)
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


def create_from_device(L):
    """A context from a device image behind a producer stream, gz_set_rgb_device without one, the context's end."""
    src = dic.lay_out(fields.primaries(W, H), "uint8", "HWC")
    with Log(L) as log:
        with L.context_from_device(image_of(src, stream=PRODUCER), W, H, TARGET) as ctx:
            ctx.set_rgb_device(image_of(src))
    return log.text


def create_and_set_rgb(L):   # (tests/test_enqueue_order.py's scenario of the host path)
    rgb = fields.primaries(W, H)
    with Log(L) as log:
        with L.context(rgb, TARGET) as ctx:
            ctx.set_rgb(rgb)
    return log.text


def test_enqueue_order_of_the_device_path(L):
    got = create_from_device(L).splitlines()
    with open(os.path.join(GOLDEN, "create_from_device.txt")) as f:
        assert got == f.read().splitlines()
    with open(os.path.join(GOLDEN, "create_and_set_rgb.txt")) as f:
        host = f.read().splitlines()
    assert create_and_set_rgb(L).splitlines() == host, "the host path's recorded order moved"
    # the host path: copy, k_linear_from_rgb8, the tail up to its synchronise -- twice -- and the context's end
    sync = host.index("stream_sync s0")
    tail, end = host[2:sync + 1], host[2 * (sync + 1):]
    assert host[sync + 1:2 * (sync + 1)] == host[:sync + 1]
    # the device path: the producer is s0 here, the context's streams follow it
    def renamed(lines):
        return [" ".join("s%d" % (int(t[1:]) + 1) if t[0] == "s" and t[1:].isdigit() else t for t in ln.split()) for ln in lines]
    assert got[0] == "record e0 s0" and got[1] == "wait s1 e0"
    assert got[2].startswith("launch k_ingest_rgb grid ") and got[2].endswith(" block 256 s1"), got[2]
    n = len(tail)
    assert got[3:3 + n] == renamed(tail), "behind the ingest: the host path's tail and its synchronise"
    # gz_set_rgb_device with producer_stream = NULL: no record / wait pair
    assert got[3 + n] == got[2] and got[4 + n:4 + 2 * n] == renamed(tail)
    assert got[4 + 2 * n:] == renamed(end)
    assert sum(ln.startswith(("record ", "wait ")) for ln in got) == 2
    assert not [ln for ln in got if ln.startswith("memcpy ") or "k_linear_from_rgb8" in ln]


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
    buf = np.zeros(64 * 64 * 3, np.uint8)
    out = np.zeros(64 * 64 * 3, np.uint8)
    good = dict(ptr=buf.ctypes.data, dtype=capi.GZ_DT_U8, strides=(192, 3, 1))

    def img(**kw):
        a = dict(good, **kw)
        return device_image(a["ptr"], a["dtype"], a["strides"])

    def create(image, w=64, h=64):
        err = C.c_int(0)
        ctx = lib.gz_create_from_device(0, w, h, C.byref(image) if image is not None else None, 1.0, C.byref(err))
        assert not ctx
        return err.value

    def pack_rc(image, w=64, h=64, dst=out):
        return lib.gz_pack_rgb_device(0, C.byref(image) if image is not None else None, w, h, dst.ctypes.data if dst is not None else None)

    wrong_size = img()
    wrong_size.struct_size -= 8
    too_far = img(strides=(1 << 57, 3, 1))          # 63 rows of 2^57 elements: the last offset needs more than 62 bits
    bad = [None, img(ptr=0), wrong_size, img(dtype=-1), img(dtype=4), img(strides=(-192, 3, 1)), img(strides=(192, -3, 1)),
           img(strides=(192, 3, -1)), too_far, img(strides=(0, 0, 1 << 61))]
    for image in bad:
        assert create(image) == -1
        assert pack_rc(image) == -1
    for w, h in ((7, 64), (64, 7), (1 << 16, 64), (64, 1 << 16), (0, 64)):    # gz_create's limits
        assert create(img(), w, h) == -1
    for w, h in ((0, 64), (64, 0), (1 << 16, 64), (64, 1 << 16), (-1, 64)):   # gz_pack_rgb_device's: 0 < w, h < 65536
        assert pack_rc(img(), w, h) == -1
    assert pack_rc(img(), dst=None) == -1
    assert lib.gz_set_rgb_device(None, C.byref(img())) == -1
    err = C.c_int(0)   # gz_create(..., NULL, ...) stays an argument error
    assert not lib.gz_create(0, 16, 16, None, 1.0, C.byref(err)) and err.value == -1
    if not has_gpu():   # valid arguments: the device is asked for, and there is none -- no fallback
        assert create(img()) == -2
        assert pack_rc(img()) == -2
        assert pack_rc(img(), 3, 5) == -2


# ------------------------------------------------------------------ the Python dispatch ----
from fake_device import FakeDeviceAddress as FakeDeviceArray  # noqa: E402


class StubHost:
    def __init__(self):
        self.calls = []

    def process(self, rgb, **kw):
        self.calls.append(("process", type(rgb).__name__, kw))
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


def test_dispatch_refuses_what_it_cannot_place(stub):
    import guetzli_amd
    with pytest.raises(ValueError, match="ambiguous"):
        guetzli_amd.process(FakeDeviceArray((3, 17, 3), "|u1"))
    with pytest.raises(TypeError):
        guetzli_amd.process(FakeDeviceArray((20, 17, 3), "<i4"))
    with pytest.raises(ValueError):
        guetzli_amd.process(FakeDeviceArray((20, 17, 4), "|u1"))
    assert stub.calls == []


def test_dispatch_of_device_arrays_and_layouts(stub):
    import guetzli_amd
    ptr = 0x7F0000000000
    assert guetzli_amd.process(FakeDeviceArray((20, 17, 3), "|u1"), quality=90)[0] == b"device"
    assert guetzli_amd.process(FakeDeviceArray((3, 20, 17), "<f4"))[0] == b"device"
    assert guetzli_amd.process(FakeDeviceArray((3, 17, 3), "<f2"), layout="CHW")[0] == b"device"
    assert guetzli_amd.process(FakeDeviceArray((20, 17), "|u1"))[0] == b"device"
    assert [c[1] for c in stub.calls] == [(ptr, 17, 20, "uint8", (51, 3, 1)), (ptr, 17, 20, "float32", (17, 1, 340)),
                                          (ptr, 3, 17, "float16", (3, 1, 51)), (ptr, 17, 20, "uint8", (17, 1, 0))]
    assert stub.calls[0][2]["quality"] == 90 and stub.calls[0][2]["stream"] == 0 and stub.calls[0][2]["device"] == 0


def test_dispatch_of_producer_streams(stub):
    """The interface's stream entry: None and 1 (the legacy default stream, which the context's blocking streams follow by
    themselves) hand nothing over; a handle is handed over, 2 (the per-thread default stream) included -- but not to
    process_many's worker threads, where 2 would name another stream; stream= overrides."""
    import guetzli_amd
    shape = (20, 17, 3)
    for given, handed in ((None, 0), (1, 0), (2, 2), (0x5EED0, 0x5EED0)):
        guetzli_amd.process(FakeDeviceArray(shape, "|u1", given))
        assert stub.calls[-1][2]["stream"] == handed, given
    guetzli_amd.process(FakeDeviceArray(shape, "|u1", 2), stream=0)
    assert stub.calls[-1][2]["stream"] == 0
    n = len(stub.calls)
    with pytest.raises(ValueError, match="per-thread"):
        guetzli_amd.process_many([FakeDeviceArray(shape, "|u1", 0x5EED0), FakeDeviceArray(shape, "|u1", 2)])
    assert len(stub.calls) == n
    out = guetzli_amd.process_many([FakeDeviceArray(shape, "|u1", 0x5EED0 + k) for k in range(5)], workers=3, quality=90)
    assert [o[0] for o in out] == [b"device"] * 5
    assert sorted(c[2]["stream"] for c in stub.calls[n:]) == [0x5EED0 + k for k in range(5)]
    assert all(c[2]["quality"] == 90 for c in stub.calls[n:])
    with pytest.raises(ValueError, match="stream="):
        guetzli_amd.process(images.crop(40, 33), stream=5)


def test_host_pixels_take_the_old_path(stub):
    import guetzli_amd
    import torch
    rgb = images.crop(40, 33)
    assert guetzli_amd.process(torch.from_numpy(rgb))[0] == b"host"
    assert guetzli_amd.process(rgb, quality=90.0, device=0)[0] == b"host"
    assert [c[0] for c in stub.calls] == ["process", "process"]
    assert stub.calls[0][1] == "Tensor" and stub.calls[1][2] == {"quality": 90.0, "device": 0}


# ------------------------------------------------------------------ bounds, under the host sanitizers ----
def test_ingest_reads_stay_inside_the_source(tmp_path):
    """tests/cpp/ingest_bounds.cc: gz_pack_rgb_device on sources malloc'ed to exactly the last addressed element + 1, every
    layout x element type x width, built as a plain program with AddressSanitizer and UBSan (unoptimised: the whole
    emulated library is its one translation unit)."""
    exe = str(tmp_path / "ingest_bounds")
    subprocess.run(["g++", "-O0", "-std=c++17", "-ffp-contract=off", "-DGZ_EMU", "-DGZ_NO_PROBES", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-w", "-I" + os.path.join(ROOT, "tests", "emu"), "-x", "c++",
                    os.path.join(ROOT, "tests", "cpp", "ingest_bounds.cc"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "924 cases, all bytes as expected" in out.stdout


if __name__ == "__main__":   # records the device path's enqueue order (only for a change that is meant to alter it)
    lib_ = Library(build_emu.build())
    lib_.lib.gz_emu_enqueue_log_fetch.restype = C.c_long
    lib_.lib.gz_emu_enqueue_log_fetch.argtypes = [C.c_char_p, C.c_long]
    text_ = create_from_device(lib_)
    with open(os.path.join(GOLDEN, "create_from_device.txt"), "w") as f_:
        f_.write(text_)
    print("create_from_device", len(text_.splitlines()), "lines")
