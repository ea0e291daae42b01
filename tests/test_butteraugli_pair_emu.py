"""The image-pair metric (gz_compare_device_pixels / gz_compare_rgb / gz_distmap_device / gz_probe_emit_map, and
guetzli_amd.butteraugli / Comparator above them) without a GPU: the kernels through the CPU emulation, where "device
memory" is host memory; the argument checks, which come before any device call; the stream contract as the emulation's
enqueue log lists it; launches and allocations failing in turn; the emit kernel's bounds under the host sanitizers.
The cases shared with the GPU suite are in tests/butteraugli_pair_cases.py.  CPU only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(HERE, "emu")]
import build_emu  # noqa: E402
import butteraugli_pair_cases as bpc  # noqa: E402
import device_input_cases as dic  # noqa: E402
from checkers import assert_bits_equal, bits, oracle, ref  # noqa: E402
from guetzli_amd import capi  # noqa: E402
from guetzli_amd.capi import GuetzliAmdError, Library, device_map, device_pixels  # noqa: E402

needs_ref = pytest.mark.skipif(ref is None, reason="oracle/_ref/libgz_ref.so not built")
CHECKERS = [pytest.param(oracle, id="oracle"), pytest.param(ref, id="ref", marks=needs_ref)]
MEM = bpc.HostMemory()
PRODUCER, CONSUMER = 0x5EED0, 0x5EED8   # stream handles of the caller's: the emulation only names them
CONFIG_IDS = ["patch2_ahead", "three_streams", "one_stream"]


@pytest.fixture(scope="module")
def L():
    lib = Library(build_emu.build())
    lib.lib.gz_emu_enqueue_log_fetch.restype = C.c_long
    lib.lib.gz_emu_enqueue_log_fetch.argtypes = [C.c_char_p, C.c_long]
    lib.lib.gz_emu_fail_alloc.argtypes = [C.c_long]
    lib.lib.gz_emu_alloc_calls.restype = C.c_long
    lib.lib.gz_emu_live.argtypes = [C.POINTER(C.c_long)] * 4
    lib.lib.gz_emu_fail_launch.argtypes = [C.c_long]
    lib.lib.gz_emu_launch_calls.restype = C.c_long
    return lib


# ------------------------------------------------------------------ the cases shared with the GPU suite ----
@pytest.mark.parametrize("chk", CHECKERS)
def test_pair_parity_at_every_size(L, chk):
    bpc.case_pair_parity_every_size(L, MEM, chk)


@pytest.mark.parametrize("chk", CHECKERS)
def test_pair_parity_of_every_pair_and_swapped(L, chk):
    bpc.case_pair_parity_every_pair(L, MEM, chk)


@pytest.mark.parametrize("dtype", bpc.dac.DTYPES)
def test_every_way_in(L, dtype):
    bpc.case_every_way_in(L, MEM, ref or oracle, dtype)


@pytest.mark.parametrize("layout", bpc.MAP_LAYOUTS)
@pytest.mark.parametrize("dtype", bpc.MAP_DTYPES)
def test_map_emit_alone(L, dtype, layout):
    bpc.case_map_emit_alone(L, MEM, dtype, layout)


@pytest.mark.parametrize("dtype", bpc.MAP_DTYPES)
def test_rounding_over_the_float32_domain(L, dtype):
    bpc.case_rounding(L, MEM, dtype)


def test_the_rounding_rules_are_torchs():
    """(of the numpy restatement the other tests compare against) float16 and bfloat16 of the rounding plane as torch
    converts them, NaN as NaN."""
    import torch
    plane = bpc.rounding_plane()
    t = torch.from_numpy(plane)
    nan = np.isnan(plane)
    for dtype, tt in (("float16", torch.float16), ("bfloat16", torch.bfloat16)):
        got = t.to(tt).view(torch.int16).numpy().view(np.uint16)
        exp = bpc.emitted_map(plane, dtype)
        assert np.array_equal(got[~nan], exp[~nan]), dtype
        assert np.isnan(bpc.widen_map(got[nan], dtype)).all()
    assert bpc.emitted_map(np.float32([1e-6]), "float16")[0] == 0x0011          # a float16 subnormal


@pytest.mark.parametrize("frame", [1, 2])
@pytest.mark.parametrize("config", bpc.CONFIGS, ids=CONFIG_IDS)
def test_state_around_a_pixel_comparison(L, config, frame):
    bpc.case_state(L, MEM, ref or oracle, config, frame)


def test_distmap_device_follows_the_last_stored_map(L):
    bpc.case_distmap_device(L, MEM)


def test_a_pending_compare_refuses_pixel_comparisons(L):
    bpc.case_pending_compare_refuses(L, MEM)


# ------------------------------------------------------------------ arguments ----
def bad_maps(w, h, ptr):
    def m(**kw):
        a = dict(dict(ptr=ptr, dtype=capi.GZ_DT_F32, strides=(w, 1)), **kw)
        return device_map(a["ptr"], a["dtype"], a["strides"])
    wrong_size = m()
    wrong_size.struct_size -= 8
    return [m(ptr=0), wrong_size, m(dtype=capi.GZ_DT_U8), m(dtype=capi.GZ_DT_U16), m(dtype=-1), m(dtype=5),
            m(strides=(-w, 1)), m(strides=(w, -1)),                       # negative
            m(strides=(0, 1)), m(strides=(w, 0)), m(strides=(1, 1)),        # a stride of 0, elements on each other
            m(strides=(w - 1, 1)), m(strides=(1, h - 1)),                   # rows / columns that overlap by one element
            m(strides=(1 << 59, 1)), m(strides=(w, 1 << 59))]               # the last offset needs more than 62 bits


def bad_pixels(w, h, ptr):
    def p(**kw):
        a = dict(dict(ptr=ptr, dtype=capi.GZ_DT_U8, strides=(3 * w, 3, 1)), **kw)
        return device_pixels(a["ptr"], a["dtype"], a["strides"])
    wrong_size = p()
    wrong_size.struct_size -= 8
    return [p(ptr=0), wrong_size, p(dtype=-1), p(dtype=5), p(strides=(-3 * w, 3, 1)), p(strides=(3 * w, -3, 1)),
            p(strides=(3 * w, 3, -1)), p(strides=(1 << 59, 3, 1))]


def test_argument_errors_come_before_any_device_call(L):
    lib = L.lib
    w, h = 33, 17
    rgb0, rgb1 = bpc.pair("photo", w, h)
    dist = np.zeros(1, np.float32)
    out = np.zeros((h, w), np.float32)
    plane = np.zeros((h, w), np.float32)
    good_px = device_pixels(rgb1.ctypes.data, capi.GZ_DT_U8, (3 * w, 3, 1))
    good_map = device_map(out.ctypes.data, capi.GZ_DT_F32, (w, 1))
    with L.context(rgb0, bpc.TARGET) as ctx:
        launches, allocs = lib.gz_emu_launch_calls(), lib.gz_emu_alloc_calls()
        with bpc_log(L) as log:
            for px in bad_pixels(w, h, rgb1.ctypes.data):
                assert lib.gz_compare_device_pixels(ctx.handle, C.byref(px), dist.ctypes.data, None) == -1
                assert lib.gz_compare_device_pixels(ctx.handle, C.byref(px), dist.ctypes.data, C.byref(good_map)) == -1
            assert lib.gz_compare_device_pixels(ctx.handle, None, dist.ctypes.data, None) == -1
            assert lib.gz_compare_device_pixels(ctx.handle, C.byref(good_px), None, None) == -1
            assert lib.gz_compare_device_pixels(None, C.byref(good_px), dist.ctypes.data, None) == -1
            for dm in bad_maps(w, h, out.ctypes.data):
                assert lib.gz_compare_device_pixels(ctx.handle, C.byref(good_px), dist.ctypes.data, C.byref(dm)) == -1
                assert lib.gz_distmap_device(ctx.handle, C.byref(dm)) == -1
                assert lib.gz_probe_emit_map(0, plane.ctypes.data, w, h, C.byref(dm)) == -1
            assert lib.gz_distmap_device(ctx.handle, None) == -1 and lib.gz_distmap_device(None, C.byref(good_map)) == -1
            assert lib.gz_compare_rgb(None, rgb1.ctypes.data, dist.ctypes.data, None) == -1
            assert lib.gz_compare_rgb(ctx.handle, None, dist.ctypes.data, None) == -1
            assert lib.gz_compare_rgb(ctx.handle, rgb1.ctypes.data, None, None) == -1
            assert lib.gz_probe_emit_map(0, None, w, h, C.byref(good_map)) == -1
            assert lib.gz_probe_emit_map(0, plane.ctypes.data, w, h, None) == -1
            for ww, hh in ((0, h), (w, 0), (1 << 16, h), (w, 1 << 16), (-1, h)):
                assert lib.gz_probe_emit_map(0, plane.ctypes.data, ww, hh, C.byref(good_map)) == -1
        assert lib.gz_emu_launch_calls() == launches and lib.gz_emu_alloc_calls() == allocs
        assert log.text == "", log.text                                   # no copy, no event, no synchronise either
        assert not out.any()
        # a dimension of one element addresses nothing: its stride does not count
        assert lib.gz_probe_emit_map(0, plane.ctypes.data, w, 1, C.byref(device_map(out.ctypes.data, capi.GZ_DT_F32, (0, 1)))) == 0
        # ... and the context is as it was
        assert bits(np.float32(ctx.compare_device_pixels(good_px, good_map))) == bits(bpc.expected(oracle, rgb0, rgb1)[0])
        assert_bits_equal(out, bpc.expected(oracle, rgb0, rgb1)[1], "map")


class bpc_log:
    """with bpc_log(L) as log: ... -> log.text, the emulation's enqueue log (tests/test_enqueue_order.py)."""

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


def test_the_product_library_checks_arguments_without_a_device():
    from guetzli_amd import build as gzbuild
    lib = Library(gzbuild.build()).lib
    w, h = 33, 17
    out = np.zeros((h, w), np.float32)
    plane = np.zeros((h, w), np.float32)
    for dm in bad_maps(w, h, out.ctypes.data):
        assert lib.gz_probe_emit_map(0, plane.ctypes.data, w, h, C.byref(dm)) == -1
        assert lib.gz_distmap_device(None, C.byref(dm)) == -1
    good = device_map(out.ctypes.data, capi.GZ_DT_F16, (w, 1))
    assert lib.gz_distmap_device(None, C.byref(good)) == -1
    assert lib.gz_compare_rgb(None, out.ctypes.data, out.ctypes.data, None) == -1
    assert lib.gz_compare_device_pixels(None, None, out.ctypes.data, None) == -1
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:   # valid arguments: the device is asked for, and there is none -- no fallback
        assert lib.gz_probe_emit_map(0, plane.ctypes.data, w, h, C.byref(good)) == -2


# ------------------------------------------------------------------ streams ----
def test_the_stream_contract_of_both_images(L):
    """The producer's stream of `other` is waited for in front of the ingest kernel; the consumer's stream of the map is
    waited for in front of the emit kernel and waits for it behind it; the call synchronises for the distance.  With
    neither: no event beyond the chain's own."""
    w, h = 33, 17
    rgb0, rgb1 = bpc.pair("photo", w, h)
    out = np.zeros((h, w), np.float32)
    with L.context(rgb0, bpc.TARGET) as ctx:
        ctx.set_config(single_stream=1)        # (the chain itself then records and waits for nothing)
        ctx.compare_rgb(rgb1)                  # (first use: the landing buffer)
        with bpc_log(L) as log:
            ctx.compare_device_pixels(device_pixels(rgb1.ctypes.data, capi.GZ_DT_U8, (3 * w, 3, 1), PRODUCER),
                                      device_map(out.ctypes.data, capi.GZ_DT_F32, (w, 1), CONSUMER))
        lines = log.text.splitlines()
        kinds = [ln.split()[0] + (" " + ln.split()[1] if ln.startswith("launch") else "") for ln in lines]
        ingest = [i for i, k in enumerate(kinds) if k == "launch k_ingest_rgb"]
        emit = [i for i, k in enumerate(kinds) if k == "launch k_emit_map"]
        rec = [i for i, k in enumerate(kinds) if k == "record"]
        wait = [i for i, k in enumerate(kinds) if k == "wait"]
        assert len(ingest) == len(emit) == 1 and len(rec) == len(wait) == 3, log.text
        lib_stream = lines[ingest[0]].split()[-1]
        assert lines[emit[0]].split()[-1] == lib_stream
        producer, consumer = lines[rec[0]].split()[-1], lines[rec[1]].split()[-1]
        assert len({producer, consumer, lib_stream}) == 3
        # the producer: recorded, waited for by the library's stream, then the ingest kernel
        assert rec[0] < wait[0] < ingest[0] and lines[wait[0]].split()[1] == lib_stream
        assert lines[rec[0]].split()[1] == lines[wait[0]].split()[2]
        # the consumer, before: recorded and waited for between the chain and the emit kernel
        assert ingest[0] < rec[1] < wait[1] < emit[0] and lines[wait[1]].split()[1] == lib_stream
        # ... and behind: the library's stream recorded, the consumer's waits
        assert emit[0] < rec[2] < wait[2] and lines[rec[2]].split()[-1] == lib_stream and lines[wait[2]].split()[1] == consumer
        assert lines[rec[2]].split()[1] == lines[wait[2]].split()[2]
        assert kinds[-1] == "stream_sync" and lines[-1].split()[-1] == lib_stream   # for the distance
        with bpc_log(L) as log:
            ctx.compare_device_pixels(device_pixels(rgb1.ctypes.data, capi.GZ_DT_U8, (3 * w, 3, 1)),
                                      device_map(out.ctypes.data, capi.GZ_DT_F32, (w, 1)))
        kinds = [ln.split()[0] for ln in log.text.splitlines()]
        assert "record" not in kinds and "wait" not in kinds and kinds[-1] == "stream_sync"
        # gz_distmap_device: with a consumer it returns behind the enqueue, without one it waits
        with bpc_log(L) as log:
            ctx.distmap_device(device_map(out.ctypes.data, capi.GZ_DT_F32, (w, 1), CONSUMER))
        kinds = [ln.split()[0] for ln in log.text.splitlines()]
        assert kinds == ["record", "wait", "launch", "record", "wait"], log.text
        with bpc_log(L) as log:
            ctx.distmap_device(device_map(out.ctypes.data, capi.GZ_DT_F32, (w, 1)))
        assert [ln.split()[0] for ln in log.text.splitlines()] == ["launch", "stream_sync"], log.text


# ------------------------------------------------------------------ launches and allocations that fail ----
def live(lib):
    v = [C.c_long() for _ in range(4)]
    lib.gz_emu_live(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)   # device bytes, page-locked bytes, blocks, events


W, H = 33, 17


def steady_context(L, rgb0):
    """A context whose lin[] is the candidate's (patch_reconstruct = 2: a Compare that trusts the planes checks them)."""
    ctx = L.context(rgb0, bpc.TARGET)
    ctx.set_config(patch_reconstruct=2)
    ctx.encode_rgb(download=False)
    ctx.quantize(bpc.Q, download=False)
    ctx.compare()
    return ctx


def pair_calls(rgb1, out):
    px = device_pixels(rgb1.ctypes.data, capi.GZ_DT_U8, (3 * W, 3, 1), PRODUCER)
    dm = device_map(out.ctypes.data, capi.GZ_DT_BF16, (W, 1), CONSUMER)
    return {"compare_device_pixels": lambda ctx: ctx.compare_device_pixels(px, dm),
            "compare_device_pixels, no map": lambda ctx: ctx.compare_device_pixels(px),
            "compare_rgb": lambda ctx: ctx.compare_rgb(rgb1)[0]}


@pytest.mark.parametrize("which", ["compare_device_pixels", "compare_device_pixels, no map", "compare_rgb"])
def test_every_launch_failing_in_turn(L, which):
    """The call fails with GZ_E_HIP, the next gz_compare trusts nothing stale and is a fresh context's bit for bit, the
    call repeated gives the checker's distance, gz_destroy leaves nothing allocated."""
    lib = L.lib
    rgb0, rgb1 = bpc.pair("photo", W, H)
    out = np.zeros((H, W), np.uint16)
    call = pair_calls(rgb1, out)[which]
    ed = bpc.expected(oracle, rgb0, rgb1)[0]
    base = live(lib)
    with steady_context(L, rgb0) as ctx:
        exp = ctx.compare()
        before = lib.gz_emu_launch_calls()
        assert bits(np.float32(call(ctx))) == bits(ed)
        n_launches = lib.gz_emu_launch_calls() - before
    assert n_launches >= 10 and live(lib) == base
    for n in range(n_launches):
        with steady_context(L, rgb0) as ctx:
            lib.gz_emu_fail_launch(n)
            try:
                with pytest.raises(GuetzliAmdError, match="GZ_E_HIP"):
                    call(ctx)
            finally:
                lib.gz_emu_fail_launch(-1)
            with pytest.raises(GuetzliAmdError, match="GZ_E_STATE"):
                ctx.distmap_device(device_map(out.ctypes.data, capi.GZ_DT_BF16, (W, 1)))
            patched_before = L.compare_counters()[0]
            got = ctx.compare()
            assert L.compare_counters()[0] == patched_before, f"launch {n} failed, and the next Compare trusted the patched planes"
            for g, e, what in zip(got, exp, ("distance", "distance map", "block maxima")):
                assert_bits_equal(np.asarray(g, np.float32), np.asarray(e, np.float32), f"{what} after launch {n} failed")
            assert bits(np.float32(call(ctx))) == bits(ed), n
        assert live(lib) == base, f"launch {n} failing leaves {live(lib)} behind"


def test_every_allocation_failing_in_turn(L):
    """The first pixel comparison of a context makes its landing buffer and its events: each failing in turn is
    GZ_E_NOMEM (or GZ_E_HIP), the same context repeats the call with the checker's bits, nothing is left allocated."""
    lib = L.lib
    rgb0, rgb1 = bpc.pair("photo", W, H)
    out = np.zeros((H, W), np.uint16)
    ed, em = bpc.expected(oracle, rgb0, rgb1)
    base = live(lib)
    for which, call in pair_calls(rgb1, out).items():
        with L.context(rgb0, bpc.TARGET) as ctx:
            before = lib.gz_emu_alloc_calls()
            call(ctx)
            n_allocs = lib.gz_emu_alloc_calls() - before
        assert n_allocs >= 1 and live(lib) == base
        for n in range(n_allocs):
            with L.context(rgb0, bpc.TARGET) as ctx:
                lib.gz_emu_fail_alloc(n)
                try:
                    with pytest.raises(GuetzliAmdError, match="GZ_E_NOMEM|GZ_E_HIP"):
                        call(ctx)
                finally:
                    lib.gz_emu_fail_alloc(-1)
                assert bits(np.float32(call(ctx))) == bits(ed), (which, n)
                if which == "compare_device_pixels":
                    assert np.array_equal(out, bpc.emitted_map(em, "bfloat16"))
            assert live(lib) == base, f"{which}: allocation {n} failing leaves {live(lib)} behind"
    # the context-free probe: its plane comes from the pool and goes back on every path
    plane = bpc.plane_of_distances(W, H, 1)
    dm = device_map(out.ctypes.data, capi.GZ_DT_BF16, (W, 1), CONSUMER)
    lib.gz_emu_fail_alloc(0)
    try:
        assert lib.gz_probe_emit_map(0, plane.ctypes.data, W, H, C.byref(dm)) == -5
    finally:
        lib.gz_emu_fail_alloc(-1)
    lib.gz_emu_fail_launch(0)
    try:
        assert lib.gz_probe_emit_map(0, plane.ctypes.data, W, H, C.byref(dm)) == -3
    finally:
        lib.gz_emu_fail_launch(-1)
    assert live(lib) == base
    L.probe_emit_map(plane, dm)
    assert np.array_equal(out, bpc.emitted_map(plane, "bfloat16"))


# ------------------------------------------------------------------ the Python surface ----
import fake_device  # noqa: E402
from fake_device import FakeDeviceArray  # noqa: E402


@pytest.fixture()
def emulated(monkeypatch, L):
    """guetzli_amd.butteraugli / Comparator on the emulated library, with numpy memory for the maps they allocate."""
    from guetzli_amd import encoder
    monkeypatch.setattr(encoder, "_pair_library", lambda: L)
    fake_device.install(monkeypatch)


def test_butteraugli_and_comparator(emulated):
    import guetzli_amd
    w, h = 33, 17
    rgb0, rgb1 = bpc.pair("photo", w, h)
    ed, em = bpc.expected(oracle, rgb0, rgb1)
    d = guetzli_amd.butteraugli(rgb0, rgb1)
    assert isinstance(d, float) and bits(np.float32(d)) == bits(ed)
    d, m = guetzli_amd.butteraugli(rgb0, rgb1, distmap=True)
    assert bits(np.float32(d)) == bits(ed)
    assert_bits_equal(m.array, em, "butteraugli(distmap=True) of host pixels")
    # device-resident images of other dtypes and layouts, a crop view for the map
    f16 = dic.from_bytes(rgb1, "float16").view(np.float16)
    chw = np.ascontiguousarray(dic.from_bytes(rgb0, "float32").transpose(2, 0, 1))
    canvas = np.full((h + 4, w + 9), 7, np.float16)
    view = canvas[2:2 + h, 5:5 + w]
    d, m = guetzli_amd.butteraugli(FakeDeviceArray(chw), FakeDeviceArray(f16), distmap=FakeDeviceArray(view, strides=view.strides))
    assert bits(np.float32(d)) == bits(ed)
    assert np.array_equal(view.view(np.uint16), bpc.emitted_map(em, "float16"))
    canvas[2:2 + h, 5:5 + w] = 7
    assert (canvas == 7).all()
    with guetzli_amd.Comparator(rgb0) as cmp:
        for name in bpc.PAIRS[1:]:
            other = bpc.pair(name, w, h)[1]
            xd, xm = bpc.expected(oracle, rgb0, other)
            d, m = cmp.compare(FakeDeviceArray(other), distmap=True)
            assert bits(np.float32(d)) == bits(xd), name
            assert_bits_equal(m.array, xm, name)
            assert bits(np.float32(cmp.compare(other))) == bits(xd)
    with pytest.raises(ValueError, match="closed"):
        cmp.compare(rgb1)
    # RGBA over a background, as process() blends it
    rgba = np.concatenate([rgb1, bpc.images.noise(w, h, seed=9)[:, :, :1]], -1)
    blended = guetzli_amd.blend_on_background(rgba, bpc.BACKGROUND)
    d = guetzli_amd.butteraugli(rgb0, FakeDeviceArray(rgba), background=bpc.BACKGROUND)
    assert bits(np.float32(d)) == bits(bpc.expected(oracle, rgb0, blended)[0])


def test_butteraugli_refuses(emulated, L):
    import guetzli_amd
    w, h = 33, 17
    rgb0, rgb1 = bpc.pair("photo", w, h)
    launches, allocs = L.lib.gz_emu_launch_calls(), L.lib.gz_emu_alloc_calls()
    with pytest.raises(ValueError, match="differ in size"):
        guetzli_amd.butteraugli(rgb0, rgb1[:, :-1])
    with pytest.raises(ValueError, match="8 x 8"):
        guetzli_amd.butteraugli(rgb0[:7], rgb1[:7])
    a = np.zeros((h, w), np.float32)
    with pytest.raises(ValueError, match="negative strides"):
        guetzli_amd.butteraugli(rgb0, rgb1, distmap=FakeDeviceArray(a, strides=(4 * w, -4)))
    with pytest.raises(ValueError, match="share an address"):
        guetzli_amd.butteraugli(rgb0, rgb1, distmap=FakeDeviceArray(a, strides=(0, 4)))
    with pytest.raises(ValueError, match="shape"):
        guetzli_amd.butteraugli(rgb0, rgb1, distmap=FakeDeviceArray(np.zeros((w, h), np.float32)))
    with pytest.raises(ValueError, match="read-only"):
        guetzli_amd.butteraugli(rgb0, rgb1, distmap=FakeDeviceArray(a, readonly=True))
    with pytest.raises(TypeError):
        guetzli_amd.butteraugli(rgb0, rgb1, distmap=FakeDeviceArray(np.zeros((h, w), np.uint8)))
    with pytest.raises(TypeError):
        guetzli_amd.butteraugli(rgb0, rgb1, distmap=a)                    # host memory is no destination
    assert (L.lib.gz_emu_launch_calls(), L.lib.gz_emu_alloc_calls()) == (launches, allocs)
    assert not a.any()


# ------------------------------------------------------------------ bounds, under the host sanitizers ----
def test_map_emit_stays_inside_its_buffers(tmp_path):
    """tests/cpp/emit_map_bounds.cc: k_emit_map through its launch code, from planes and into destinations malloc'ed to
    exactly the last addressed element + 1, every layout x element type x size x source alignment, built as a plain
    program with AddressSanitizer and UBSan.  Its own process, nothing preloaded."""
    exe = str(tmp_path / "emit_map_bounds")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-DGZ_EMU", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-w", "-I" + os.path.join(ROOT, "tests", "emu"), "-x", "c++",
                    os.path.join(ROOT, "tests", "cpp", "emit_map_bounds.cc"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "810 cases, all elements as expected, no access outside the buffers" in out.stdout
