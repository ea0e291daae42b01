"""Butteraugli's masking on the device (gz_opsin_device / gz_mask_device / gz_adaptive_quantization, and
guetzli_amd.opsin_dynamics / mask / adaptive_quantization above them) without a GPU: the kernels through the CPU
emulation, where "device memory" is host memory; launches and allocations failing in turn; what runs and what does not
for the quantisation field, and the stream contract, as the emulation's enqueue log lists them.
The cases shared with the GPU suite are in tests/mask_cases.py.  CPU only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "emu")]
import build_emu  # noqa: E402
import butteraugli_linear_cases as blc  # noqa: E402
import butteraugli_pair_cases as bpc  # noqa: E402
import mask_cases as mc  # noqa: E402
from checkers import assert_bits_equal, oracle, ref  # noqa: E402
from guetzli_amd import capi  # noqa: E402
from guetzli_amd.capi import GZ_SAMPLES_LINEAR, GuetzliAmdError, Library, device_map, device_output, device_pixels  # noqa: E402

needs_ref = pytest.mark.skipif(ref is None, reason="oracle/_ref/libgz_ref.so not built")
CHECKERS = [pytest.param(oracle, id="oracle"), pytest.param(ref, id="ref", marks=needs_ref)]
CHK = ref or oracle
MEM = bpc.HostMemory()
PRODUCER, PRODUCER1, CONSUMER, CONSUMER1 = 0x5EED0, 0x5EED4, 0x5EED8, 0x5EEDC   # stream handles of the caller's: the emulation only names them


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
def test_the_quantisation_field_is_the_references(L, chk):
    mc.case_quant_parity(L, MEM, chk)


@pytest.mark.parametrize("chk", CHECKERS)
def test_mask_of_pairs_in_both_orders_and_of_one_image(L, chk):
    mc.case_mask_parity(L, MEM, chk)


@pytest.mark.parametrize("chk", CHECKERS)
def test_the_opsin_image_is_the_references(L, chk):
    mc.case_opsin_parity(L, MEM, chk)


@pytest.mark.parametrize("dtype", mc.DTYPES)
def test_every_way_out(L, dtype):
    assert mc.case_every_way_out(L, MEM, CHK, dtype) == {"wide", "elementwise"}


@pytest.mark.parametrize("dtype", mc.DTYPES)
def test_every_way_in(L, dtype):
    assert mc.case_every_way_in(L, MEM, CHK, dtype) == {"planar", "interleaved", "elementwise"}


def test_clamp_and_count(L):
    mc.case_clamp_and_count(L, MEM, CHK)


# ------------------------------------------------------------------ the enqueue log ----
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

    def launches(self, name):
        """The grids (x, y, z) of the launches of kernel `name`, in order."""
        return [tuple(int(v) for v in ln.split()[3].split("x")) for ln in self.text.splitlines() if ln.split()[:2] == ["launch", name]]

    def kinds(self):
        return [ln.split()[0] + (" " + ln.split()[1] if ln.startswith("launch") else "") for ln in self.text.splitlines()]


W, H = 33, 17


def arguments(w=W, h=H, producer=0, producer1=0, consumer=0, consumer1=0):
    a, b = blc.noise_pair(w, h)
    sa, sb = blc.image_of_planes(a, "float32"), blc.image_of_planes(b, "float32")
    out = {k: np.zeros(s, np.float32) for k, s in (("xyb", (3, h, w)), ("mask", (3, h, w)), ("dc", (3, h, w)), ("quant", (h, w)))}
    pa = device_pixels(sa.ctypes.data, capi.GZ_DT_F32, (3 * w, 3, 1), producer)
    pb = device_pixels(sb.ctypes.data, capi.GZ_DT_F32, (3 * w, 3, 1), producer1)
    chw = (w, 1, w * h)
    dest = {"xyb": device_output(out["xyb"].ctypes.data, capi.GZ_DT_F32, chw, consumer),
            "mask": device_output(out["mask"].ctypes.data, capi.GZ_DT_F32, chw, consumer),
            "dc": device_output(out["dc"].ctypes.data, capi.GZ_DT_F32, chw, consumer1),
            "quant": device_map(out["quant"].ctypes.data, capi.GZ_DT_F32, (w, 1), consumer)}
    return a, b, pa, pb, out, dest, (sa, sb)


def test_the_quantisation_field_runs_half_of_masks_first_stage(L):
    """One gz_adaptive_quantization call: one k_mask_pre launch of ONE plane (grid z = 1: Y in slot 0, no X-plane block),
    no paired column pass (grid z = 2) and, behind the context's creation, no two-plane radius-20 row pass; the Y-only
    emit.  gz_mask_device of the same image, beside it, runs both planes."""
    a, b, pa, pb, out, dest, keep = arguments()
    with enqueue_log(L) as full:
        L.mask_device(pa, None, W, H, dest["mask"], dest["dc"], GZ_SAMPLES_LINEAR)
    with enqueue_log(L) as quant:
        L.adaptive_quantization(pa, W, H, dest["quant"])
    columns = ("k_blur_v_compact", "k_blur_v_pk")
    assert [g[2] for g in full.launches("k_mask_pre")] == [2]
    assert sum(g[2] == 2 for k in columns for g in full.launches(k)) == 1          # the paired radius-20 pass
    assert [g[2] for g in quant.launches("k_mask_pre")] == [1]
    assert not any(g[2] == 2 for k in columns for g in quant.launches(k))
    rows = lambda log: sum(len(log.launches(k)) for k in ("k_blur_h", "k_blur_h_pk"))
    both = lambda log: sum(g[2] == 2 for k in ("k_blur_h", "k_blur_h_pk") for g in log.launches(k))
    assert rows(quant) == rows(full) and both(quant) == both(full) - 1               # the same passes, one of them on one plane
    assert len(quant.launches("k_emit_mask")) == 1 and len(full.launches("k_emit_mask")) == 1
    assert not quant.launches("k_combine") and not full.launches("k_combine")      # no mask planes in between
    assert_bits_equal(out["quant"], mc.expected_quant(oracle, a), "quantisation field")
    assert_bits_equal(out["mask"], mc.expected_mask(oracle, a, a)[0], "mask")


def test_the_stream_contract(L):
    """Every producer's stream is waited for in front of its ingest kernel; each consumer's stream in front of the emit
    kernel, and it waits behind it; the call ends with its own synchronise."""
    a, b, pa, pb, out, dest, keep = arguments(producer=PRODUCER, producer1=PRODUCER1, consumer=CONSUMER, consumer1=CONSUMER1)
    with enqueue_log(L) as log:
        L.mask_device(pa, pb, W, H, dest["mask"], dest["dc"], GZ_SAMPLES_LINEAR)
    kinds = log.kinds()
    ingest = [i for i, k in enumerate(kinds) if k == "launch k_ingest_linear"]
    emit = [i for i, k in enumerate(kinds) if k == "launch k_emit_mask"]
    rec = [i for i, k in enumerate(kinds) if k == "record"]
    wait = [i for i, k in enumerate(kinds) if k == "wait"]
    assert len(ingest) == 2 and len(emit) == 1, log.text
    # two producers, two consumers in front, two consumers behind: each a record and a wait, in this order
    assert len(rec) == len(wait) == 6, log.text
    assert rec[0] < wait[0] < ingest[0] < rec[1] < wait[1] < ingest[1] < rec[2] < wait[2] < rec[3] < wait[3] < emit[0] < rec[4] < wait[4] < rec[5] < wait[5]
    lines = log.text.splitlines()
    own = lines[ingest[0]].split()[-1]                         # the context's stream
    assert [lines[i].split()[1] for i in wait[:4]] == [own] * 4 and all(lines[i].split()[1] != own for i in wait[4:]), log.text
    assert kinds[-1] == "stream_sync" or "stream_sync" in kinds[wait[5]:], log.text
    assert_bits_equal(out["mask"], mc.expected_mask(oracle, a, b)[0], "mask")
    assert_bits_equal(out["dc"], mc.expected_mask(oracle, a, b)[1], "mask_dc")
    for name, call in (("xyb", lambda d: L.opsin_device(pa, W, H, d, GZ_SAMPLES_LINEAR)), ("quant", lambda d: L.adaptive_quantization(pa, W, H, d))):
        with enqueue_log(L) as log:
            call(dest[name])
        kinds = log.kinds()
        first = min(i for i, k in enumerate(kinds) if k.startswith("launch k_emit"))
        last = max(i for i, k in enumerate(kinds) if k.startswith("launch k_emit"))
        rec = [i for i, k in enumerate(kinds) if k == "record"]
        wait = [i for i, k in enumerate(kinds) if k == "wait"]
        assert len(rec) == len(wait) == 3, log.text
        assert rec[0] < wait[0] < kinds.index("launch k_ingest_linear") < rec[1] < wait[1] < first <= last < rec[2] < wait[2], log.text
    assert_bits_equal(out["xyb"], mc.expected_opsin(oracle, a), "opsin image")
    assert_bits_equal(out["quant"], mc.expected_quant(oracle, a), "quantisation field")


# ------------------------------------------------------------------ launches and allocations that fail ----
def live(lib):
    v = [C.c_long() for _ in range(4)]
    lib.gz_emu_live(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)   # device bytes, page-locked bytes, blocks, events


def failing_calls():
    """name -> (call(L), check()): every new entry."""
    a, b, pa, pb, out, dest, keep = arguments(17, 16, PRODUCER, PRODUCER1, CONSUMER, CONSUMER1)

    def check_mask():
        assert_bits_equal(out["mask"], mc.expected_mask(oracle, a, b)[0], "mask")
        assert_bits_equal(out["dc"], mc.expected_mask(oracle, a, b)[1], "mask_dc")

    return {"opsin": (lambda L: L.opsin_device(pa, 17, 16, dest["xyb"], GZ_SAMPLES_LINEAR),
                      lambda: assert_bits_equal(out["xyb"], mc.expected_opsin(oracle, a), "opsin image")),
            "mask": (lambda L: L.mask_device(pa, pb, 17, 16, dest["mask"], dest["dc"], GZ_SAMPLES_LINEAR), check_mask),
            "quant": (lambda L: L.adaptive_quantization(pa, 17, 16, dest["quant"]),
                      lambda: assert_bits_equal(out["quant"], mc.expected_quant(oracle, a), "quantisation field"))}, (out, keep)


@pytest.mark.parametrize("which", ["opsin", "mask", "quant"])
def test_every_launch_and_allocation_failing_in_turn(L, which):
    """Each launch and each allocation of the call failing in turn: an error code, nothing left allocated, and the call
    repeated gives the checker's planes."""
    lib = L.lib
    calls, (out, keep) = failing_calls()
    call, check = calls[which]
    base = live(lib)
    launches, allocs = lib.gz_emu_launch_calls(), lib.gz_emu_alloc_calls()
    call(L)
    check()
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
    for o in out.values():
        o[...] = 0
    call(L)
    check()


# ------------------------------------------------------------------ the Python surface ----
import fake_device  # noqa: E402
from fake_device import FakeDeviceArray  # noqa: E402


@pytest.fixture()
def emulated(monkeypatch, L):
    """guetzli_amd.opsin_dynamics / mask / adaptive_quantization on the emulated library, with numpy memory for what they
    allocate."""
    from guetzli_amd import encoder
    monkeypatch.setattr(encoder, "_pair_library", lambda: L)
    fake_device.install(monkeypatch)


def test_the_python_functions(emulated):
    import guetzli_amd
    w, h = 33, 17
    a, b = blc.noise_pair(w, h)
    em, edc = mc.expected_mask(oracle, a, b)
    # host arrays, CHW float32 in 0..255 and in [0, 1]
    assert_bits_equal(guetzli_amd.opsin_dynamics(a, linear=True).array, mc.expected_opsin(oracle, a), "opsin_dynamics")
    m = guetzli_amd.mask(a, b, linear=True)
    assert_bits_equal(m.array, em, "mask")
    m, dc = guetzli_amd.mask(a, b, dc=True, linear=True, layout="HWC")
    assert_bits_equal(m.array, em.transpose(1, 2, 0), "mask, HWC")
    assert_bits_equal(dc.array, edc.transpose(1, 2, 0), "mask_dc, HWC")
    a01 = a / np.float32(255)
    q = guetzli_amd.adaptive_quantization(a01, scale=255)
    assert_bits_equal(q.array, mc.expected_quant(oracle, a01 * np.float32(255)), "adaptive_quantization(scale=255)")
    # 8-bit host pixels; one image with itself
    rgb0, rgb1 = bpc.pair("photo", w, h)
    l0, l1 = blc.fields.linear(rgb0), blc.fields.linear(rgb1)
    assert_bits_equal(guetzli_amd.mask(rgb0, rgb1).array, mc.expected_mask(oracle, l0, l1)[0], "mask of bytes")
    assert_bits_equal(guetzli_amd.mask(rgb0).array, mc.expected_mask(oracle, l0, l0)[0], "mask of an image with itself")
    assert_bits_equal(guetzli_amd.opsin_dynamics(rgb0).array, mc.expected_opsin(oracle, l0), "opsin_dynamics of bytes")
    # out= as a crop view of a float16 canvas
    canvas = np.full((h + 4, w + 9), 7, np.float16)
    view = canvas[2:2 + h, 5:5 + w]
    got = guetzli_amd.adaptive_quantization(FakeDeviceArray(a), out=FakeDeviceArray(view, strides=view.strides))
    assert got.array is view
    assert np.array_equal(view.view(np.uint16), bpc.emitted_map(mc.expected_quant(oracle, a), "float16"))
    canvas[2:2 + h, 5:5 + w] = 7
    assert (canvas == 7).all()
    # strict
    bad = a.copy()
    bad[1, 2, 3] = np.nan
    bad[0, 0, 0] = 300
    guetzli_amd.adaptive_quantization(bad)
    for call in (lambda: guetzli_amd.adaptive_quantization(bad, strict=True), lambda: guetzli_amd.opsin_dynamics(bad, linear=True, strict=True)):
        with pytest.raises(ValueError, match="2 elements"):
            call()
    with pytest.raises(ValueError, match="4 elements"):
        guetzli_amd.mask(bad, bad, linear=True, strict=True)


def test_the_python_functions_refuse_before_any_device_work(emulated, L):
    import guetzli_amd
    a, _ = blc.noise_pair(33, 17)
    launches, allocs = L.lib.gz_emu_launch_calls(), L.lib.gz_emu_alloc_calls()
    with pytest.raises(ValueError, match="16 x 16"):
        guetzli_amd.adaptive_quantization(a[:, :, :15])
    with pytest.raises(ValueError, match="16 x 16"):
        guetzli_amd.adaptive_quantization(a[:, :15, :16])
    with pytest.raises(ValueError, match="8 x 8"):
        guetzli_amd.mask(a[:, :7], linear=True)
    with pytest.raises(ValueError, match="8 x 8"):
        guetzli_amd.opsin_dynamics(a[:, :, :7], linear=True)
    with pytest.raises(ValueError, match="differ in size"):
        guetzli_amd.mask(a, a[:, :, :-1], linear=True)
    with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
        guetzli_amd.adaptive_quantization(a.astype(np.uint8))
    with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
        guetzli_amd.mask(a, linear=True, out=FakeDeviceArray(np.zeros((3, 17, 33), np.uint8)))
    with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
        guetzli_amd.opsin_dynamics(a, linear=True, dtype="uint8")
    with pytest.raises(ValueError, match="share an address"):
        guetzli_amd.adaptive_quantization(a, out=FakeDeviceArray(np.zeros((17, 33), np.float32), strides=(0, 4)))
    with pytest.raises(ValueError, match="background"):
        guetzli_amd.mask(a, linear=True, background=0)
    assert (L.lib.gz_emu_launch_calls(), L.lib.gz_emu_alloc_calls()) == (launches, allocs)


# ------------------------------------------------------------------ bounds, under the host sanitizers ----
def test_the_emit_kernel_stays_inside_its_buffers(tmp_path):
    """tests/cpp/emit_mask_bounds.cc: k_emit_mask through its launch code, in every mode, from blurred planes and a table
    malloc'ed to their exact sizes into destinations malloc'ed to exactly the last addressed element + 1 -- every layout
    x element type x width -- built as a plain program with AddressSanitizer and UBSan.  Its own process, nothing
    preloaded."""
    import subprocess
    root = os.path.dirname(HERE)
    exe = str(tmp_path / "emit_mask_bounds")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-DGZ_EMU", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-w", "-I" + os.path.join(root, "tests", "emu"), "-x", "c++",
                    os.path.join(root, "tests", "cpp", "emit_mask_bounds.cc"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all elements as expected, no access outside the buffers" in out.stdout
