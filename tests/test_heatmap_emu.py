"""Butteraugli's heat map (gz_heatmap_device / gz_compare_device_pixels_heat / gz_heatmap_from_map_device /
gz_probe_emit_heat, the threshold table behind them, gz_butteraugli_fuzzy_*, and guetzli_amd.heatmap / butteraugli /
Comparator above them) without a GPU: the kernel through the CPU emulation, where "device memory" is host memory; the
table builder against the process's own pow; the argument checks, which come before any device call; the stream
contract as the emulation's enqueue log lists it; launches and allocations failing in turn; the kernel's bounds under
the host sanitizers.  The cases shared with the GPU suite are in tests/heatmap_cases.py.  CPU only."""
import ctypes as C
import math
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
import device_output_cases as doc  # noqa: E402
import heatmap_cases as hc  # noqa: E402
from checkers import assert_bits_equal, bits, oracle, ref  # noqa: E402
from guetzli_amd import capi  # noqa: E402
from guetzli_amd.capi import GuetzliAmdError, Library, device_map, device_output, device_pixels  # noqa: E402

MEM = bpc.HostMemory()
PRODUCER, CONSUMER = 0x5EED0, 0x5EED8   # stream handles of the caller's: the emulation only names them
GOOD, BAD = hc.default_thresholds()
THRESHOLDS = [pytest.param((GOOD, BAD), id="default"), pytest.param(hc.OTHER_THRESHOLDS, id="other")]


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


class Log:
    """with Log(L) as log: ... -> log.text, the emulation's enqueue log (tests/test_enqueue_order.py)."""

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


# ------------------------------------------------------------------ the table and the thresholds ----
def host_byte(v):
    return int(255 * math.pow(v, 0.5) + 0.5)


def test_the_threshold_table_is_the_hosts_pow(L):
    """The builder's own condition, restated: over the 129 doubles within 64 ulps of ((k - 0.5) / 255)^2 the byte of the
    process's pow does not decrease, starts at k - 1, ends at k and changes once -- and thr[k] is where it changes."""
    thr = L.probe_heat_thresholds()
    assert thr.shape == (255,) and (np.diff(thr) > 0).all() and 0 < thr[0] and thr[-1] < 1
    for k in range(1, 256):
        v = ((k - 0.5) / 255) * ((k - 0.5) / 255)
        for _ in range(64):
            v = math.nextafter(v, 0.0)
        window = [v]
        for _ in range(128):
            window.append(math.nextafter(window[-1], 2.0))
        b = [host_byte(x) for x in window]
        assert b[0] == k - 1 and b[-1] == k and all(y - x in (0, 1) for x, y in zip(b, b[1:])) and b.count(k) + b.count(k - 1) == 129, k
        assert window[b.index(k)] == thr[k - 1], k
    assert L.lib.gz_probe_heat_thresholds(None) == -1


def test_the_fuzzy_functions_are_the_restatements(L):
    for s in np.linspace(0, 4, 1001):
        assert L.fuzzy_class(float(s)) == hc.fuzzy_class(float(s))
    for seek in (0.5, 1.0, 1.5, 0.1, 1.9, 0.840253347958):
        assert L.fuzzy_inverse(seek) == hc.fuzzy_inverse(seek)
    assert L.default_heat_thresholds() == (GOOD, BAD)
    assert 0.76 < GOOD < 0.77 and 1.14 < BAD < 1.15


# ------------------------------------------------------------------ the cases shared with the GPU suite ----
@pytest.mark.parametrize("thresholds", THRESHOLDS)
def test_every_synthetic_distance(L, thresholds):
    hc.case_probe_values(L, MEM, *thresholds)


def test_the_references_recorded_heat_map(L):
    hc.case_golden(L, MEM, GOOD, BAD)


@pytest.mark.parametrize("layout", hc.LAYOUTS)
@pytest.mark.parametrize("dtype", hc.DTYPES)
def test_probe_at_every_shape(L, dtype, layout):
    paths = hc.case_probe_shapes(L, MEM, dtype, layout, GOOD, BAD)
    assert paths == EXPECTED_PATHS[layout], paths


# which instantiations of the kernel a layout reaches over the sizes (16-byte stores need aligned rows: in a contiguous
# image only some widths have them; a crop's canvas has them at every width)
EXPECTED_PATHS = {"HWC": {"interleaved", "elementwise"}, "CHW": {"planar", "elementwise"}, "HWC_crop": {"interleaved"},
                  "CHW_crop": {"planar"}, "HWC_base1": {"elementwise"}, "CHW_crop_base1": {"elementwise"},
                  "HWC_pitch1": {"interleaved", "elementwise"}, "WHC": {"elementwise"}}


@pytest.mark.parametrize("layout", hc.LAYOUTS)
@pytest.mark.parametrize("dtype", ["uint8", "float32", "bfloat16"])
def test_the_context_free_entry_at_every_shape(L, dtype, layout):
    hc.case_from_map_shapes(L, MEM, dtype, layout, GOOD, BAD)


def test_compare_with_a_heat_map(L):
    hc.case_compare_with_heat(L, MEM, ref or oracle, GOOD, BAD)


def test_heatmap_device_follows_the_last_stored_map(L):
    hc.case_state(L, MEM, GOOD, BAD)


# ------------------------------------------------------------------ arguments ----
def bad_outputs(w, h, ptr):
    def o(**kw):
        a = dict(dict(ptr=ptr, dtype=capi.GZ_DT_U8, strides=(3 * w, 3, 1)), **kw)
        return device_output(a["ptr"], a["dtype"], a["strides"])
    wrong_size = o()
    wrong_size.struct_size -= 8
    return [o(ptr=0), wrong_size, o(dtype=-1), o(dtype=5),
            o(strides=(-3 * w, 3, 1)), o(strides=(3 * w, -3, 1)), o(strides=(3 * w, 3, -1)),          # negative
            o(strides=(0, 3, 1)), o(strides=(3 * w, 0, 1)), o(strides=(3 * w, 3, 0)),                 # a stride of 0
            o(strides=(3 * w - 1, 3, 1)), o(strides=(3 * w, 2, 1)), o(strides=(w, 1, w * h - 1)),      # elements on each other
            o(strides=(1 << 59, 3, 1))]                                                              # more than 62 bits


BAD_THRESHOLDS = [(0.0, 1.0), (-1.0, 1.0), (1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (1.0, float("nan")), (1.0, float("inf")),
                  (float("inf"), float("inf"))]


def test_argument_errors_come_before_any_device_call(L):
    lib = L.lib
    w, h = 33, 17
    rgb0, rgb1 = bpc.pair("photo", w, h)
    dist = np.zeros(1, np.float32)
    heat = np.zeros((h, w, 3), np.uint8)
    plane = np.ones((h, w), np.float32)
    px = device_pixels(rgb1.ctypes.data, capi.GZ_DT_U8, (3 * w, 3, 1))
    good_out = device_output(heat.ctypes.data, capi.GZ_DT_U8, (3 * w, 3, 1))
    with L.context(rgb0, bpc.TARGET) as ctx:
        ctx.compare_rgb(rgb1)                                             # (a map is stored: nothing below is refused for its lack)
        launches, allocs = lib.gz_emu_launch_calls(), lib.gz_emu_alloc_calls()
        with Log(L) as log:
            calls = {
                "gz_heatmap_device": lambda out, g, b: lib.gz_heatmap_device(ctx.handle, g, b, out),
                "gz_compare_device_pixels_heat": lambda out, g, b: lib.gz_compare_device_pixels_heat(ctx.handle, C.byref(px), dist.ctypes.data, None, out, g, b),
                "gz_heatmap_from_map_device": lambda out, g, b: lib.gz_heatmap_from_map_device(0, plane.ctypes.data, w, h, w, g, b, out),
                "gz_probe_emit_heat": lambda out, g, b: lib.gz_probe_emit_heat(0, plane.ctypes.data, w, h, g, b, out)}
            for name, call in calls.items():
                for out in bad_outputs(w, h, heat.ctypes.data):
                    assert call(C.byref(out), GOOD, BAD) == -1, name
                for g, b in BAD_THRESHOLDS:
                    assert call(C.byref(good_out), g, b) == -1, (name, g, b)
            assert lib.gz_heatmap_device(ctx.handle, GOOD, BAD, None) == -1 and lib.gz_heatmap_device(None, GOOD, BAD, C.byref(good_out)) == -1
            assert lib.gz_compare_device_pixels_heat(None, C.byref(px), dist.ctypes.data, None, C.byref(good_out), GOOD, BAD) == -1
            assert lib.gz_compare_device_pixels_heat(ctx.handle, None, dist.ctypes.data, None, C.byref(good_out), GOOD, BAD) == -1
            assert lib.gz_compare_device_pixels_heat(ctx.handle, C.byref(px), None, None, C.byref(good_out), GOOD, BAD) == -1
            assert lib.gz_heatmap_from_map_device(0, None, w, h, w, GOOD, BAD, C.byref(good_out)) == -1
            assert lib.gz_heatmap_from_map_device(0, plane.ctypes.data, w, h, w - 1, GOOD, BAD, C.byref(good_out)) == -1
            assert lib.gz_probe_emit_heat(0, None, w, h, GOOD, BAD, C.byref(good_out)) == -1
            for ww, hh in ((0, h), (w, 0), (1 << 16, h), (w, 1 << 16), (-1, h)):
                assert lib.gz_probe_emit_heat(0, plane.ctypes.data, ww, hh, GOOD, BAD, C.byref(good_out)) == -1
                assert lib.gz_heatmap_from_map_device(0, plane.ctypes.data, ww, hh, max(ww, 1), GOOD, BAD, C.byref(good_out)) == -1
        assert lib.gz_emu_launch_calls() == launches and lib.gz_emu_alloc_calls() == allocs
        assert log.text == "", log.text                                   # no copy, no event, no synchronise either
        assert not heat.any() and dist[0] == 0
        # ... and the context is as it was: the stored map is still there
        ctx.heatmap_device(GOOD, BAD, good_out)
        assert np.array_equal(heat, hc.expected_heat(bpc.expected(oracle, rgb0, rgb1)[1], GOOD, BAD))


def test_the_product_library_checks_arguments_without_a_device():
    from guetzli_amd import build as gzbuild
    Lp = Library(gzbuild.build())
    lib = Lp.lib
    w, h = 33, 17
    heat = np.zeros((h, w, 3), np.uint8)
    plane = np.ones((h, w), np.float32)
    good_out = device_output(heat.ctypes.data, capi.GZ_DT_U8, (3 * w, 3, 1))
    for out in bad_outputs(w, h, heat.ctypes.data):
        assert lib.gz_probe_emit_heat(0, plane.ctypes.data, w, h, GOOD, BAD, C.byref(out)) == -1
        assert lib.gz_heatmap_from_map_device(0, plane.ctypes.data, w, h, w, GOOD, BAD, C.byref(out)) == -1
    for g, b in BAD_THRESHOLDS:
        assert lib.gz_probe_emit_heat(0, plane.ctypes.data, w, h, g, b, C.byref(good_out)) == -1
    assert lib.gz_heatmap_device(None, GOOD, BAD, C.byref(good_out)) == -1
    # the host side of the device library: the same table, the same thresholds, no device
    assert np.array_equal(Lp.probe_heat_thresholds(), Library(build_emu.build()).probe_heat_thresholds())
    assert Lp.default_heat_thresholds() == (GOOD, BAD)
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:   # valid arguments: the device is asked for, and there is none -- no fallback
        assert lib.gz_probe_emit_heat(0, plane.ctypes.data, w, h, GOOD, BAD, C.byref(good_out)) == -2


# ------------------------------------------------------------------ streams ----
def kinds_of(text):
    return [ln.split()[0] + (" " + ln.split()[1] if ln.startswith("launch") else "") for ln in text.splitlines()]


def test_the_stream_contract_of_the_heat_map(L):
    """The consumer's stream of the heat map is waited for in front of k_emit_heat and waits for it behind it, as for the
    map; with one, gz_heatmap_device returns behind the enqueue, without one it waits."""
    w, h = 33, 17
    rgb0, rgb1 = bpc.pair("photo", w, h)
    heat = np.zeros((h, w, 3), np.uint8)
    out = np.zeros((h, w), np.float32)
    px = device_pixels(rgb1.ctypes.data, capi.GZ_DT_U8, (3 * w, 3, 1), PRODUCER)
    with L.context(rgb0, bpc.TARGET) as ctx:
        ctx.set_config(single_stream=1)        # (the chain itself then records and waits for nothing)
        ctx.compare_device_pixels_heat(px, device_output(heat.ctypes.data, capi.GZ_DT_U8, (3 * w, 3, 1)), GOOD, BAD)   # (first use: the tables)
        with Log(L) as log:
            ctx.compare_device_pixels_heat(px, device_output(heat.ctypes.data, capi.GZ_DT_U8, (3 * w, 3, 1), CONSUMER), GOOD, BAD,
                                           device_map(out.ctypes.data, capi.GZ_DT_F32, (w, 1), CONSUMER))
        lines = log.text.splitlines()
        kinds = kinds_of(log.text)
        ingest, emap, eheat = (kinds.index("launch " + k) for k in ("k_ingest_rgb", "k_emit_map", "k_emit_heat"))
        rec = [i for i, k in enumerate(kinds) if k == "record"]
        wait = [i for i, k in enumerate(kinds) if k == "wait"]
        assert len(rec) == len(wait) == 5, log.text      # the producer; the consumer before and behind each of the two kernels
        lib_stream = lines[ingest].split()[-1]
        assert lines[emap].split()[-1] == lib_stream and lines[eheat].split()[-1] == lib_stream
        consumer = lines[rec[1]].split()[-1]
        assert ingest < rec[1] < wait[1] < emap < rec[2] < wait[2] < rec[3] < wait[3] < eheat < rec[4] < wait[4]
        assert lines[rec[3]].split()[-1] == consumer and lines[wait[3]].split()[1] == lib_stream
        assert lines[rec[4]].split()[-1] == lib_stream and lines[wait[4]].split()[1] == consumer
        assert lines[rec[4]].split()[1] == lines[wait[4]].split()[2]
        assert kinds[-1] == "stream_sync" and lines[-1].split()[-1] == lib_stream   # for the distance
        with Log(L) as log:
            ctx.heatmap_device(GOOD, BAD, device_output(heat.ctypes.data, capi.GZ_DT_U8, (3 * w, 3, 1), CONSUMER))
        assert [ln.split()[0] for ln in log.text.splitlines()] == ["record", "wait", "launch", "record", "wait"], log.text
        with Log(L) as log:
            ctx.heatmap_device(GOOD, BAD, device_output(heat.ctypes.data, capi.GZ_DT_U8, (3 * w, 3, 1)))
        assert [ln.split()[0] for ln in log.text.splitlines()] == ["launch", "stream_sync"], log.text
    # the context-free entry: the consumer before the tables are written and behind the kernel, and its own wait
    plane = hc.plane_of_size(w, h, GOOD, BAD, seed=1)
    with Log(L) as log:
        L.heatmap_from_map_device(plane.ctypes.data, w, h, w, GOOD, BAD, device_output(heat.ctypes.data, capi.GZ_DT_U8, (3 * w, 3, 1), CONSUMER))
    kinds = [ln.split()[0] for ln in log.text.splitlines()]
    assert kinds.index("record") < kinds.index("wait") < kinds.index("launch") < len(kinds) - 1 - kinds[::-1].index("record")
    assert kinds.count("record") == kinds.count("wait") == 2 and kinds[-1] == "stream_sync", log.text
    assert np.array_equal(heat, hc.expected_heat(plane, GOOD, BAD))


# ------------------------------------------------------------------ launches and allocations that fail ----
def live(lib):
    v = [C.c_long() for _ in range(4)]
    lib.gz_emu_live(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)   # device bytes, page-locked bytes, blocks, events


W, H = 33, 17


def steady_context(L, rgb0):
    ctx = L.context(rgb0, bpc.TARGET)
    ctx.set_config(patch_reconstruct=2)
    ctx.encode_rgb(download=False)
    ctx.quantize(bpc.Q, download=False)
    ctx.compare()
    return ctx


def heat_calls(rgb1, heat):
    px = device_pixels(rgb1.ctypes.data, capi.GZ_DT_U8, (3 * W, 3, 1), PRODUCER)
    out = device_output(heat.ctypes.data, capi.GZ_DT_BF16, (W, 1, W * H), CONSUMER)
    return {"compare_device_pixels_heat": lambda ctx: ctx.compare_device_pixels_heat(px, out, GOOD, BAD),
            "heatmap_device": lambda ctx: ctx.heatmap_device(GOOD, BAD, out)}


@pytest.mark.parametrize("which", ["compare_device_pixels_heat", "heatmap_device"])
def test_every_launch_and_allocation_failing_in_turn(L, which):
    """The call fails with GZ_E_HIP / GZ_E_NOMEM.  gz_heatmap_device changes no claim: the stored map is still the
    one gz_distmap_device writes, and the call repeated gives its heat map.  A failed comparison trusts nothing stale:
    the next gz_compare is a fresh context's bit for bit.  gz_destroy leaves nothing allocated."""
    lib = L.lib
    rgb0, rgb1 = bpc.pair("photo", W, H)
    heat = np.zeros((3, H, W), np.uint16)
    call = heat_calls(rgb1, heat)[which]
    em = bpc.expected(oracle, rgb0, rgb1)[1]
    base = live(lib)
    with steady_context(L, rgb0) as ctx:
        exp = ctx.compare()
        launches, allocs = lib.gz_emu_launch_calls(), lib.gz_emu_alloc_calls()
        call(ctx)
        n_launches, n_allocs = lib.gz_emu_launch_calls() - launches, lib.gz_emu_alloc_calls() - allocs
    want = doc.emitted(hc.expected_heat(em if which == "compare_device_pixels_heat" else exp[1], GOOD, BAD), "bfloat16").transpose(2, 0, 1)
    assert np.array_equal(heat, want)
    assert n_launches >= 1 and n_allocs >= 1 and live(lib) == base
    for fail, n_calls, code in ((lib.gz_emu_fail_launch, n_launches, "GZ_E_HIP"), (lib.gz_emu_fail_alloc, n_allocs, "GZ_E_NOMEM|GZ_E_HIP")):
        for n in range(n_calls):
            with steady_context(L, rgb0) as ctx:
                heat[...] = 0
                fail(n)
                try:
                    with pytest.raises(GuetzliAmdError, match=code):
                        call(ctx)
                finally:
                    fail(-1)
                if which == "heatmap_device":   # no claim changed: the map is there, and is the candidate's
                    got = np.zeros((H, W), np.float32)
                    ctx.distmap_device(device_map(got.ctypes.data, capi.GZ_DT_F32, (W, 1)))
                    assert_bits_equal(got, exp[1], f"the stored map after failure {n}")
                got = ctx.compare()
                for g, e, what in zip(got, exp, ("distance", "distance map", "block maxima")):
                    assert_bits_equal(np.asarray(g, np.float32), np.asarray(e, np.float32), f"{what} after failure {n} ({code})")
                call(ctx)
                assert np.array_equal(heat, want), n
            assert live(lib) == base, f"failure {n} ({code}) leaves {live(lib)} behind"


def test_the_context_free_entries_give_everything_back(L):
    lib = L.lib
    plane = hc.plane_of_size(W, H, GOOD, BAD, seed=2)
    heat = np.zeros((H, W, 3), np.uint8)
    out = device_output(heat.ctypes.data, capi.GZ_DT_U8, (3 * W, 3, 1), CONSUMER)
    lib.gz_trim_pool()     # (nothing cached: every block and event the entries take is a real allocation)
    base = live(lib)
    entries = {"probe": lambda: lib.gz_probe_emit_heat(0, plane.ctypes.data, W, H, GOOD, BAD, C.byref(out)),
               "from_map": lambda: lib.gz_heatmap_from_map_device(0, plane.ctypes.data, W, H, W, GOOD, BAD, C.byref(out))}
    for name, entry in entries.items():
        allocs = lib.gz_emu_alloc_calls()
        assert entry() == 0
        n_allocs = lib.gz_emu_alloc_calls() - allocs
        lib.gz_trim_pool()
        assert n_allocs >= 1 and live(lib) == base
        for n in range(n_allocs):
            lib.gz_trim_pool()
            lib.gz_emu_fail_alloc(n)
            try:
                assert entry() in (-5, -3), (name, n)
            finally:
                lib.gz_emu_fail_alloc(-1)
            lib.gz_trim_pool()
            assert live(lib) == base, (name, n, live(lib))
        lib.gz_emu_fail_launch(0)
        try:
            assert entry() == -3
        finally:
            lib.gz_emu_fail_launch(-1)
        heat[...] = 0
        assert entry() == 0 and np.array_equal(heat, hc.expected_heat(plane, GOOD, BAD))
        lib.gz_trim_pool()
        assert live(lib) == base


# ------------------------------------------------------------------ the Python surface ----
import fake_device  # noqa: E402
from fake_device import FakeDeviceArray  # noqa: E402


@pytest.fixture()
def emulated(monkeypatch, L):
    """guetzli_amd.butteraugli / Comparator / heatmap on the emulated library, with numpy memory for what they allocate."""
    from guetzli_amd import encoder
    monkeypatch.setattr(encoder, "_pair_library", lambda: L)
    fake_device.install(monkeypatch)


def test_the_python_surface(emulated):
    import guetzli_amd
    w, h = 33, 17
    rgb0, rgb1 = bpc.pair("photo", w, h)
    ed, em = bpc.expected(oracle, rgb0, rgb1)
    heat = hc.expected_heat(em, GOOD, BAD)
    assert guetzli_amd.fuzzy_inverse(1.5) == GOOD and guetzli_amd.fuzzy_class(1.0) == hc.fuzzy_class(1.0)
    # without heatmap=, return values are what they were
    assert isinstance(guetzli_amd.butteraugli(rgb0, rgb1), float)
    assert len(guetzli_amd.butteraugli(rgb0, rgb1, distmap=True)) == 2
    d, hm = guetzli_amd.butteraugli(rgb0, rgb1, heatmap=True)
    assert bits(np.float32(d)) == bits(ed) and np.array_equal(hm.array, heat)
    d, m, hm = guetzli_amd.butteraugli(rgb0, FakeDeviceArray(rgb1), distmap=True, heatmap=True)
    assert bits(np.float32(d)) == bits(ed) and np.array_equal(hm.array, heat)
    assert_bits_equal(m.array, em, "the map beside the heat map")
    # a crop view of float16 in CHW, other thresholds
    canvas = np.full((3, h + 4, w + 9), 7, np.float16)
    view = canvas[:, 2:2 + h, 5:5 + w]
    with guetzli_amd.Comparator(rgb0) as cmp:
        d, hm = cmp.compare(FakeDeviceArray(rgb1), heatmap=FakeDeviceArray(view, strides=view.strides), good=0.5, bad=2.25)
        assert bits(np.float32(d)) == bits(ed)
        assert np.array_equal(view.view(np.uint16), doc.emitted(hc.expected_heat(em, 0.5, 2.25), "float16").transpose(2, 0, 1))
        canvas[:, 2:2 + h, 5:5 + w] = 7
        assert (canvas == 7).all()
        assert isinstance(cmp.compare(rgb1), float)
    # heatmap() of a map of the caller's, rows with a pitch
    held = np.zeros((h, w + 5), np.float32)
    held[:, :w] = em
    out = np.zeros((h, w, 3), np.uint8)
    got = guetzli_amd.heatmap(FakeDeviceArray(held[:, :w], strides=held[:, :w].strides), out=FakeDeviceArray(out))
    assert np.array_equal(got.array, heat)
    # refusals, before anything runs
    with pytest.raises(ValueError, match="good"):
        guetzli_amd.butteraugli(rgb0, rgb1, heatmap=True, good=2.0, bad=1.0)
    with pytest.raises(ValueError, match="negative strides"):
        guetzli_amd.butteraugli(rgb0, rgb1, heatmap=FakeDeviceArray(out, strides=(3 * w, -3, 1)))
    with pytest.raises(ValueError, match="share an address"):
        guetzli_amd.butteraugli(rgb0, rgb1, heatmap=FakeDeviceArray(out, strides=(0, 3, 1)))
    with pytest.raises(ValueError, match="shape"):
        guetzli_amd.butteraugli(rgb0, rgb1, heatmap=FakeDeviceArray(np.zeros((w, h, 3), np.uint8)))
    with pytest.raises(ValueError, match="read-only"):
        guetzli_amd.butteraugli(rgb0, rgb1, heatmap=FakeDeviceArray(out, readonly=True))
    with pytest.raises(TypeError):
        guetzli_amd.butteraugli(rgb0, rgb1, heatmap=out)                    # host memory is no destination
    with pytest.raises(TypeError):
        guetzli_amd.heatmap(FakeDeviceArray(np.zeros((h, w), np.float64)))


# ------------------------------------------------------------------ bounds, under the host sanitizers ----
def test_heat_emit_stays_inside_its_buffers(tmp_path):
    """tests/cpp/emit_heat_bounds.cc: k_emit_heat through its launch code, from planes and into destinations malloc'ed to
    exactly the last addressed element + 1, every layout x element type x size x source alignment, built as a plain
    program with AddressSanitizer and UBSan.  Its own process, nothing preloaded."""
    exe = str(tmp_path / "emit_heat_bounds")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-DGZ_EMU", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-w", "-I" + os.path.join(ROOT, "tests", "emu"), "-x", "c++",
                    os.path.join(ROOT, "tests", "cpp", "emit_heat_bounds.cc"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "2160 cases, all elements as expected, no access outside the buffers" in out.stdout
