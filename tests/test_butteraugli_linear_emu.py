"""Butteraugli of linear float images (gz_create_from_device_linear / gz_set_linear_device / gz_compare_device_linear /
gz_butteraugli_linear, and guetzli_amd.butteraugli_linear / Comparator(linear=True) above them) without a GPU: the
kernels through the CPU emulation, where "device memory" is host memory; launches and allocations failing in turn; the
stream contract as the emulation's enqueue log lists it; the ingest kernel's bounds under the host sanitizers.
The cases shared with the GPU suite are in tests/butteraugli_linear_cases.py.  CPU only."""
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
import butteraugli_linear_cases as blc  # noqa: E402
import butteraugli_pair_cases as bpc  # noqa: E402
import device_input_cases as dic  # noqa: E402
import heatmap_cases as hc  # noqa: E402
from checkers import assert_bits_equal, bits, oracle, ref  # noqa: E402
from guetzli_amd import capi  # noqa: E402
from guetzli_amd.capi import GuetzliAmdError, Library, device_map, device_pixels  # noqa: E402

needs_ref = pytest.mark.skipif(ref is None, reason="oracle/_ref/libgz_ref.so not built")
CHECKERS = [pytest.param(oracle, id="oracle"), pytest.param(ref, id="ref", marks=needs_ref)]
CHK = ref or oracle
MEM = bpc.HostMemory()
PRODUCER, CONSUMER = 0x5EED0, 0x5EED8   # stream handles of the caller's: the emulation only names them
GOOD, BAD = hc.default_thresholds()


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
def test_parity_of_linear_pairs_and_swapped(L, chk):
    blc.case_parity(L, MEM, chk)


def test_a_difference_under_a_byte_step_has_a_distance(L):
    blc.case_the_byte_path_cannot_see_it(L, MEM, CHK)


@pytest.mark.parametrize("dtype", blc.DTYPES)
def test_every_way_in(L, dtype):
    assert blc.case_every_way_in(L, MEM, CHK, dtype) == {"planar", "interleaved", "elementwise"}


def test_clamp_and_count(L):
    blc.case_clamp_and_count(L, MEM, CHK)


def test_small_images_take_the_references_border(L):
    blc.case_small_images(L, MEM, CHK, GOOD, BAD)


def test_state_of_a_linear_context(L):
    blc.case_state(L, MEM, CHK)


def test_a_pending_compare_refuses_linear_entries(L):
    blc.case_pending_compare_refuses(L, MEM)


# ------------------------------------------------------------------ streams ----
class enqueue_log:
    """with enqueue_log(L) as log: ... -> log.text, the emulation's enqueue log (tests/test_enqueue_order.py)."""

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


def test_the_stream_contract_and_the_one_copy(L):
    """The producer's stream is waited for in front of the counter's fill and the ingest kernel; the map's consumer as
    for the 8-bit entry; ONE device-to-host copy and ONE synchronise fetch the distance and the count."""
    w, h = 33, 17
    a, b = blc.noise_pair(w, h)
    sa, sb = blc.image_of_planes(a, "float32"), blc.image_of_planes(b, "float32")
    out = np.zeros((h, w), np.float32)
    with blc.linear_context(L, MEM, dic.lay_out(sa, "float32", "HWC")) as ctx:
        ctx.set_config(single_stream=1)        # (the chain itself then records and waits for nothing)
        ctx.compare_device_linear(device_pixels(sb.ctypes.data, capi.GZ_DT_F32, (3 * w, 3, 1)))   # (first use: the events)
        with enqueue_log(L) as log:
            ctx.compare_device_linear(device_pixels(sb.ctypes.data, capi.GZ_DT_F32, (3 * w, 3, 1), PRODUCER), 1.0,
                                      device_map(out.ctypes.data, capi.GZ_DT_F32, (w, 1), CONSUMER))
        lines = log.text.splitlines()
        kinds = [ln.split()[0] + (" " + ln.split()[1] if ln.startswith("launch") else "") for ln in lines]
        ingest = [i for i, k in enumerate(kinds) if k == "launch k_ingest_linear"]
        emit = [i for i, k in enumerate(kinds) if k == "launch k_emit_map"]
        rec = [i for i, k in enumerate(kinds) if k == "record"]
        wait = [i for i, k in enumerate(kinds) if k == "wait"]
        assert len(ingest) == len(emit) == 1 and len(rec) == len(wait) == 3, log.text
        assert "launch k_ingest_rgb" not in kinds and "launch k_region_max" not in kinds
        assert rec[0] < wait[0] < ingest[0] < rec[1] < wait[1] < emit[0] < rec[2] < wait[2]
        assert kinds[ingest[0] - 1].startswith("memset"), log.text        # the counter's fill, right in front of the kernel
        copies = [k for k in kinds if k.startswith("memcpy")]
        assert len(copies) == 1 and kinds.count("stream_sync") == 1 and kinds[-1] == "stream_sync", log.text
        assert_bits_equal(out, blc.expected(oracle, a, b)[1], "map")


# ------------------------------------------------------------------ launches and allocations that fail ----
def live(lib):
    v = [C.c_long() for _ in range(4)]
    lib.gz_emu_live(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)   # device bytes, page-locked bytes, blocks, events


W, H = 17, 9
SMALL = (3, 5)


def failing_calls():
    """name -> (call(L) -> distance, the checker's distance): every new entry, on fresh contexts."""
    a, b = blc.noise_pair(W, H)
    sa, sb = blc.image_of_planes(a, "float32"), blc.image_of_planes(b, "float32")
    out = np.zeros((H, W), np.uint16)
    heat = np.zeros((H, W, 3), np.uint8)
    pa = device_pixels(sa.ctypes.data, capi.GZ_DT_F32, (3 * W, 3, 1), PRODUCER)
    pb = device_pixels(sb.ctypes.data, capi.GZ_DT_F32, (3 * W, 3, 1), PRODUCER)
    dm = device_map(out.ctypes.data, capi.GZ_DT_BF16, (W, 1), CONSUMER)
    ho = capi.device_output(heat.ctypes.data, capi.GZ_DT_U8, (3 * W, 3, 1), CONSUMER)
    sw, sh = SMALL
    ssa, ssb = np.ascontiguousarray(sa[:sh, :sw]), np.ascontiguousarray(sb[:sh, :sw])
    sout = np.zeros((sh, sw), np.float32)
    spa = device_pixels(ssa.ctypes.data, capi.GZ_DT_F32, (3 * sw, 3, 1))
    spb = device_pixels(ssb.ctypes.data, capi.GZ_DT_F32, (3 * sw, 3, 1))
    sdm = device_map(sout.ctypes.data, capi.GZ_DT_F32, (sw, 1))
    small0, small1 = blc.planes_of(ssa, "float32"), blc.planes_of(ssb, "float32")
    keep = (sa, sb, out, heat, ssa, ssb, sout)

    def create_and_compare(L):
        with L.context_from_device_linear(pa, W, H) as ctx:
            return ctx.compare_device_linear(pb, 1.0, dm, ho, GOOD, BAD)[0]

    def set_and_compare(L):
        with L.context(bpc.pair("photo", W, H)[0], bpc.TARGET) as ctx:
            ctx.set_linear_device(pa)
            return ctx.compare_device_linear(pb)[0]

    return {"create + compare": (create_and_compare, blc.expected(oracle, a, b)[0]),
            "set + compare": (set_and_compare, blc.expected(oracle, a, b)[0]),
            "butteraugli_linear": (lambda L: L.butteraugli_linear(pa, pb, W, H, 1.0, dm, ho, GOOD, BAD)[0], blc.expected(oracle, a, b)[0]),
            "butteraugli_linear, small": (lambda L: L.butteraugli_linear(spa, spb, sw, sh, 1.0, sdm)[0], blc.expected_small(oracle, small0, small1)[0])}, keep


@pytest.mark.parametrize("which", ["create + compare", "set + compare", "butteraugli_linear", "butteraugli_linear, small"])
def test_every_launch_and_allocation_failing_in_turn(L, which):
    """Each launch and each allocation of the call failing in turn: an error code, nothing left allocated, and the call
    repeated gives the checker's distance."""
    lib = L.lib
    calls, keep = failing_calls()
    call, ed = calls[which]
    base = live(lib)
    launches, allocs = lib.gz_emu_launch_calls(), lib.gz_emu_alloc_calls()
    assert bits(np.float32(call(L))) == bits(ed)
    n_launches, n_allocs = lib.gz_emu_launch_calls() - launches, lib.gz_emu_alloc_calls() - allocs
    assert n_launches >= 10 and n_allocs >= 1 and live(lib) == base
    for n in range(n_launches):
        lib.gz_emu_fail_launch(n)
        try:
            with pytest.raises(GuetzliAmdError, match="GZ_E_HIP"):
                call(L)
        finally:
            lib.gz_emu_fail_launch(-1)
        assert live(lib) == base, f"launch {n} failing leaves {live(lib)} behind"
    for n in range(n_allocs):
        lib.gz_emu_fail_alloc(n)
        try:
            with pytest.raises(GuetzliAmdError, match="GZ_E_NOMEM|GZ_E_HIP"):
                call(L)
        finally:
            lib.gz_emu_fail_alloc(-1)
        assert live(lib) == base, f"allocation {n} failing leaves {live(lib)} behind"
    assert bits(np.float32(call(L))) == bits(ed)


def test_a_failed_linear_compare_leaves_the_context_usable(L):
    """On one context: a launch of gz_compare_device_linear fails, gz_distmap_device refuses the half-written map, the
    next gz_compare of the candidate is a fresh context's, the call repeated gives the checker's distance."""
    lib = L.lib
    w, h = 33, 17
    rgb0, _ = bpc.pair("photo", w, h)
    _, b = blc.noise_pair(w, h)
    sb = blc.image_of_planes(b, "float32")
    pb = device_pixels(sb.ctypes.data, capi.GZ_DT_F32, (3 * w, 3, 1))
    out = np.zeros((h, w), np.float32)
    ed = blc.expected(oracle, blc.fields.linear(rgb0), b)[0]
    with L.context(rgb0, bpc.TARGET) as ctx:
        ctx.set_config(patch_reconstruct=2)
        ctx.encode_rgb(download=False)
        ctx.quantize(bpc.Q, download=False)
        exp = ctx.compare()
        before = lib.gz_emu_launch_calls()
        assert bits(np.float32(ctx.compare_device_linear(pb)[0])) == bits(ed)
        n_launches = lib.gz_emu_launch_calls() - before
        for n in range(0, n_launches, 3):
            ctx.compare()
            lib.gz_emu_fail_launch(n)
            try:
                with pytest.raises(GuetzliAmdError, match="GZ_E_HIP"):
                    ctx.compare_device_linear(pb, 1.0, device_map(out.ctypes.data, capi.GZ_DT_F32, (w, 1)))
            finally:
                lib.gz_emu_fail_launch(-1)
            with pytest.raises(GuetzliAmdError, match="GZ_E_STATE"):
                ctx.distmap_device(device_map(out.ctypes.data, capi.GZ_DT_F32, (w, 1)))
            got = ctx.compare()
            for g, e, what in zip(got, exp, ("distance", "distance map", "block maxima")):
                assert_bits_equal(np.asarray(g, np.float32), np.asarray(e, np.float32), f"{what} after launch {n} failed")
            assert bits(np.float32(ctx.compare_device_linear(pb)[0])) == bits(ed), n


# ------------------------------------------------------------------ the Python surface ----
import fake_device  # noqa: E402
from fake_device import FakeDeviceArray  # noqa: E402


@pytest.fixture()
def emulated(monkeypatch, L):
    """guetzli_amd.butteraugli_linear / Comparator on the emulated library, with numpy memory for what they allocate."""
    from guetzli_amd import encoder
    monkeypatch.setattr(encoder, "_pair_library", lambda: L)
    fake_device.install(monkeypatch)


def test_butteraugli_linear_and_comparator(emulated):
    import guetzli_amd
    w, h = 33, 17
    a, b = blc.noise_pair(w, h)
    ed, em = blc.expected(oracle, a, b)
    a01, b01 = a / np.float32(255), b / np.float32(255)          # CHW float32 in [0, 1], host arrays
    ea, eb = (a01 * np.float32(255)), (b01 * np.float32(255))
    xd, xm = blc.expected(oracle, ea, eb)
    d = guetzli_amd.butteraugli_linear(a, b)
    assert isinstance(d, float) and bits(np.float32(d)) == bits(ed)
    d, m = guetzli_amd.butteraugli_linear(a01, b01, scale=255, distmap=True)
    assert bits(np.float32(d)) == bits(xd)
    assert_bits_equal(m.array, xm, "butteraugli_linear(scale=255, distmap=True)")
    # device-resident: HWC float16 against CHW float32, a float16 crop view for the map, a heat map
    f16 = np.ascontiguousarray(b.transpose(1, 2, 0)).astype(np.float16)
    e16 = np.ascontiguousarray(f16.astype(np.float32).transpose(2, 0, 1))
    hd, hm = blc.expected(oracle, a, e16)
    canvas = np.full((h + 4, w + 9), 7, np.float16)
    view = canvas[2:2 + h, 5:5 + w]
    d, m, heat = guetzli_amd.butteraugli_linear(FakeDeviceArray(a), FakeDeviceArray(f16), distmap=FakeDeviceArray(view, strides=view.strides),
                                                heatmap=True)
    assert bits(np.float32(d)) == bits(hd)
    assert np.array_equal(view.view(np.uint16), bpc.emitted_map(hm, "float16"))
    assert np.array_equal(heat.array, hc.expected_heat(hm, GOOD, BAD))
    canvas[2:2 + h, 5:5 + w] = 7
    assert (canvas == 7).all()
    # 1 x 1, and a grey 3 x 5
    one0, one1 = np.float32([[[10.0, 200.0, 30.5]]]), np.float32([[[12.0, 190.0, 30.0]]])
    sd, sm = blc.expected_small(oracle, blc.planes_of(one0, "float32"), blc.planes_of(one1, "float32"))
    d, m = guetzli_amd.butteraugli_linear(one0, one1, distmap=True)
    assert bits(np.float32(d)) == bits(sd) and m.array.shape == (1, 1)
    assert_bits_equal(m.array, sm, "1 x 1")
    # strict
    bad = a.copy()
    bad[1, 2, 3] = np.nan
    bad[0, 0, 0] = 300
    assert guetzli_amd.butteraugli_linear(bad, b) >= 0
    with pytest.raises(ValueError, match="2 elements"):
        guetzli_amd.butteraugli_linear(bad, b, strict=True)
    # one reference, three images; then an 8-bit image against it
    with guetzli_amd.Comparator(a01, linear=True, scale=255) as cmp:
        for k in range(3):
            other = np.clip(b01 + np.float32(0.001 * k), 0, 1).astype(np.float32)
            od, om = blc.expected(oracle, ea, other * np.float32(255))
            d, m = cmp.compare(other, distmap=True)
            assert bits(np.float32(d)) == bits(od), k
            assert_bits_equal(m.array, om, f"Comparator(linear=True), image {k}")
            assert cmp.clamped == 0
        cmp.compare(bad / np.float32(255))
        assert cmp.clamped == 2
        rgb1 = bpc.pair("photo", w, h)[1]
        d = cmp.compare(rgb1, linear=False)
        assert bits(np.float32(d)) == bits(blc.expected(oracle, ea, blc.fields.linear(rgb1))[0]) and cmp.clamped == 0
    with guetzli_amd.Comparator(bpc.pair("photo", w, h)[0]) as cmp:       # an 8-bit reference takes a linear image too
        d = cmp.compare(b, linear=True)
        assert bits(np.float32(d)) == bits(blc.expected(oracle, blc.fields.linear(bpc.pair("photo", w, h)[0]), b)[0])


def test_butteraugli_linear_refuses(emulated, L):
    import guetzli_amd
    w, h = 33, 17
    a, b = blc.noise_pair(w, h)
    launches, allocs = L.lib.gz_emu_launch_calls(), L.lib.gz_emu_alloc_calls()
    with pytest.raises(ValueError, match="differ in size"):
        guetzli_amd.butteraugli_linear(a, b[:, :, :-1])
    with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
        guetzli_amd.butteraugli_linear(a.astype(np.uint8), b)
    with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
        guetzli_amd.butteraugli_linear(FakeDeviceArray(a.astype(np.uint8)), b)
    with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
        guetzli_amd.butteraugli_linear(a.astype(np.float64), b)
    with pytest.raises(ValueError, match="alpha is not supported"):
        guetzli_amd.butteraugli_linear(np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32))
    for scale in (0, -1, np.nan, np.inf):
        with pytest.raises(ValueError, match="scale"):
            guetzli_amd.butteraugli_linear(a, b, scale=scale)
    with pytest.raises(ValueError, match="share an address"):
        guetzli_amd.butteraugli_linear(a, b, distmap=FakeDeviceArray(np.zeros((h, w), np.float32), strides=(0, 4)))
    with pytest.raises(ValueError, match="8 x 8"):
        guetzli_amd.Comparator(a[:, :7], linear=True)
    assert (L.lib.gz_emu_launch_calls(), L.lib.gz_emu_alloc_calls()) == (launches, allocs)


# ------------------------------------------------------------------ bounds, under the host sanitizers ----
def test_linear_ingest_stays_inside_its_buffers(tmp_path):
    """tests/cpp/ingest_linear_bounds.cc: k_ingest_linear through its launch code, from sources and into planes malloc'ed
    to exactly the last addressed element + 1 -- every layout x element type x width, the extension of small images --
    and k_region_max over windows of a plane, built as a plain program with AddressSanitizer and UBSan.  Its own
    process, nothing preloaded."""
    exe = str(tmp_path / "ingest_linear_bounds")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-DGZ_EMU", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-w", "-I" + os.path.join(ROOT, "tests", "emu"), "-x", "c++",
                    os.path.join(ROOT, "tests", "cpp", "ingest_linear_bounds.cc"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all elements as expected, no access outside the buffers" in out.stdout
