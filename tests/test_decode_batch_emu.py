"""The batched device decode (gz_decode_scan_batch_device, DecodeJpegBatchToRGB, guetzli_amd.decode_batch) without a GPU:
the batched kernels of gz_kernels_scandec.h, gz_kernels_block.h and gz_kernels_emit.h through the CPU emulation, the host
driver linked against it.  Every comparison is for equality: a batch member's result is the single call's for the same
scan, its pixels are gz_decode_coeffs' of the host reader's coefficients, and decode_batch's image i is
decode(jpegs[i], entropy="host").  CPU only."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "emu")]
import build_emu  # noqa: E402
import decode_batch_cases as dbc  # noqa: E402
import device_output_cases as doc  # noqa: E402
import scan_decode_cases as sdc  # noqa: E402
from guetzli_amd import capi  # noqa: E402
from guetzli_amd.capi import GuetzliAmdError, Library, device_output, device_output_batch  # noqa: E402
from guetzli_amd.encoder import DTYPE_CODES  # noqa: E402

CONSUMER = 0x5EED0   # a stream handle of the caller's: the emulation only names it


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


@pytest.fixture(scope="module")
def host():
    from guetzli_amd.encoder import HostLibrary
    return HostLibrary(build_emu.build_host())


def live(lib):
    v = [C.c_long() for _ in range(4)]
    lib.gz_emu_live(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


_SINGLE = {}


def single(L, host, data, subseq=0, rounds=0):
    """(the single call's result for this scan, the pixels gz_decode_coeffs makes of the HOST reader's coefficients -- None where
    the status is not DECODED), computed once per stream and setting."""
    key = (data, subseq, rounds)
    if key not in _SINGLE:
        scan, j = sdc.scan_of(data, subseq, rounds)
        dest = doc.destination(j["w"], j["h"], "uint8", "HWC")
        res = L.decode_scan_device(scan, device_output(dest.address, DTYPE_CODES["uint8"], dest.strides, 0))
        rgb = None
        if res["status"] == "DECODED":
            ref = host.decode_jpeg_coeffs(data, "host")
            if ref is not None:
                rgb = L.decode_coeffs(ref[0] if j["factor"] == 2 else ref[0].reshape(3, -1, 64), j["w"], j["h"], j["factor"])
            else:   # (the host refuses what stands BEHIND a scan the device decoded: the single call's own pixels)
                rgb = dest.image_of(dest.raw).copy()
            dest.check(rgb)
        else:
            assert np.array_equal(dest.raw, dest.before)
        _SINGLE[key] = (res, rgb)
    return _SINGLE[key]


def batch(L, jpegs, subseq=0, rounds=0, dtype="uint8", layout="HWC", stream=0, scratch=0, slots=None, n_out=None):
    scans = [sdc.scan_of(d, subseq, rounds)[0] for d in jpegs]
    j = sdc.parse_jpeg(jpegs[0])
    n_out = n_out or len(jpegs)
    canvas = dbc.BatchCanvas(n_out, j["w"], j["h"], dtype, layout)
    out = device_output_batch(canvas.address, DTYPE_CODES[dtype], canvas.strides, n_out, stream)
    return L.decode_scan_batch_device(scans, slots if slots is not None else list(range(len(jpegs))), out, scratch_bytes=scratch), canvas


def check_batch(L, host, jpegs, what, subseq=0, rounds=0, **kw):
    res, canvas = batch(L, jpegs, subseq, rounds, **kw)
    want = [single(L, host, d, subseq, rounds) for d in jpegs]
    assert res == [w[0] for w in want], (what, subseq, res, [w[0] for w in want])
    slots = kw.get("slots") or list(range(len(jpegs)))
    canvas.check({slots[i]: w[1] for i, w in enumerate(want)}, what=what)
    return res


# ------------------------------------------------------------------ results and pixels are the single call's ----
@pytest.mark.parametrize("subseq", sdc.SUBSEQ)
def test_every_member_is_its_single_call(L, host, subseq):
    """Synthetic batches of every sampling (16-bit codes and short ones, quantisers that differ), 8 x 8 and 1 x 1 images, the
    256 / 257 / 1-lane streams in every order, N = 1: results[i] is gz_decode_scan_device's, the pixels in sentinel canvases are
    gz_decode_coeffs' of the host reader's coefficients, nothing outside the images is written."""
    layouts = itertools.cycle([("uint8", "HWC"), ("bfloat16", "CHW_crop_base1"), ("float32", "HWC_odd_n"), ("uint16", "HWC")])
    for name, jpegs in dbc.synthetic_batches().items():
        dtype, layout = next(layouts)
        check_batch(L, host, jpegs, name, subseq, dtype=dtype, layout=layout, stream=CONSUMER if len(name) % 2 else 0)
        check_batch(L, host, jpegs[2:3], name + " alone", subseq)
    lanes = dbc.lane_batch()
    assert {k: dbc.lanes_of(v) for k, v in lanes.items()} == {"256": 256, "257": 257, "1": 1}
    for order in itertools.permutations(["256", "257", "1"]):
        res = check_batch(L, host, [lanes[k] for k in order], order, subseq)
        if subseq == 16:
            assert [r["subsequences"] for r in res] == [int(k) for k in order]
            assert [r["sync_rounds"] for r in res] == [1 if k == "257" else 0 for k in order]


def test_slots_scatter_the_images(L, host):
    """slots[i] is the image scan i fills: a permutation into a larger batch leaves the other images untouched."""
    jpegs = dbc.synthetic_batches()["420_41x23"]
    check_batch(L, host, jpegs, "slots", slots=[5, 0, 3, 2], n_out=7, layout="CHW_crop_base1")


def test_images_converge_in_different_rounds(L, host):
    """The stream that does not synchronise inside a workgroup between two that need no round: lane 0 of its first
    workgroup enters blind whatever the image in front of it left at the boundary, the rounds are its own, and with one
    round it alone is NOT_CONVERGED, its image untouched."""
    jpegs = dbc.slow_batch()
    res = check_batch(L, host, jpegs, "slow", 16)
    assert [r["sync_rounds"] for r in res] == [0, 2, 0] and res[1]["subsequences"] > 2 * dbc.LANES, res
    res = check_batch(L, host, jpegs, "slow, one round", 16, 1)
    assert [r["status"] for r in res] == ["DECODED", "NOT_CONVERGED", "DECODED"] and [r["sync_rounds"] for r in res] == [0, 1, 0], res
    res = check_batch(L, host, [jpegs[1], jpegs[0], jpegs[1]], "slow first and last", 16)
    assert [r["sync_rounds"] for r in res] == [2, 0, 2], res


def test_a_mutated_member_changes_no_other(L, host):
    """Batches of mutated streams: every member's status is its single-call status, images whose status is not DECODED are
    untouched, the others exact.  The streams used hold at least one the host reader accepts and one it refuses."""
    name, kind, batches = next(iter(dbc.mutated_batches(140)))
    flat = [d for b in batches for d in b[1:]]
    accepted = [host.decode_jpeg_coeffs(d, "host") is not None for d in flat]
    assert any(accepted) and not all(accepted)
    statuses = set()
    for i, b in enumerate(batches):
        statuses |= {r["status"] for r in check_batch(L, host, b, (name, kind, i))}
    assert "DECODED" in statuses and statuses & set(sdc.ERROR_STATUSES), statuses


@pytest.mark.parametrize("per_chunk", [1, 2])
def test_chunks_give_the_same_results(L, host, per_chunk):
    lanes = dbc.lane_batch()
    jpegs = [lanes["257"], lanes["256"], lanes["1"], lanes["257"], lanes["256"]]
    cap = dbc.scratch_bytes([lanes["257"]] * per_chunk, 16)
    log = enqueue_log(L, lambda: check_batch(L, host, jpegs, f"chunks of {per_chunk}", 16, scratch=cap, layout="HWC_odd_n"))
    assert kernels_of(log).count("k_scandec_sync_first_batch") == -(-len(jpegs) // per_chunk), kernels_of(log)
    with pytest.raises(GuetzliAmdError, match="GZ_E_ARG"):   # a scan that does not fit alone
        batch(L, jpegs, 16, scratch=dbc.scratch_bytes([lanes["257"]], 16) - 1)


# ------------------------------------------------------------------ the enqueue log ----
def enqueue_log(L, call):
    L.lib.gz_emu_enqueue_log_start()
    try:
        call()
    finally:
        L.lib.gz_emu_enqueue_log_stop()
    n = L.lib.gz_emu_enqueue_log_fetch(None, 0)
    buf = C.create_string_buffer(n + 1)
    L.lib.gz_emu_enqueue_log_fetch(buf, n)
    return buf.raw[:n].decode().splitlines()


def kernels_of(log):
    return [ln.split()[1].strip("()").split("<")[0] for ln in log if ln.startswith("launch")]


def test_the_launches_do_not_depend_on_n(L, host):
    """A batch of N eligible images of one sampling enqueues the launches of ONE decode plus the rounds, on one stream: the
    same list for N = 2 and N = 4; the host reads N words per round and 4 N at the end."""
    jpegs = dbc.synthetic_batches()["444_40x24"]
    slow = dbc.slow_batch()
    for members, rounds, pixels in ((jpegs[:2], 0, "k_reconstruct_batch"), (jpegs, 0, "k_reconstruct_batch"), (slow[:2], 2, "k_reconstruct_batch"),
                                    (dbc.synthetic_batches()["420_41x23"], 0, "k_chroma_samples_batch k_reconstruct420_batch")):
        log = enqueue_log(L, lambda: batch(L, members, 16))
        assert {ln.split()[-1] for ln in log if ln.split()[0] in ("launch", "memcpy", "memset", "stream_sync")} == {"s0"}, log
        assert kernels_of(log) == ["k_scandec_sync_first_batch"] + ["k_scandec_sync_next_batch"] * rounds + \
            ["k_scan_offsets", "k_scandec_write_batch", "k_scandec_dc_batch"] + pixels.split() + ["k_emit_rgb"], kernels_of(log)
        d2h = [int(ln.split()[2]) for ln in log if ln.startswith("memcpy d2h")]
        assert d2h == [4 * len(members)] * rounds + [16 * len(members)], d2h


# ------------------------------------------------------------------ failures injected ----
def test_every_launch_and_allocation_failing_in_turn(L, host):
    """Each launch and each allocation of the call failing in turn: the call's error, every result at "no verdict", nothing
    left allocated, and the next call is correct.  (The slow stream and a neighbour at 16 bytes: every kernel, rounds included.)"""
    lib = L.lib
    jpegs = dbc.slow_batch()[:2]
    base = live(lib)
    launches, allocs = lib.gz_emu_launch_calls(), lib.gz_emu_alloc_calls()
    check_batch(L, host, jpegs, "before", 16, stream=CONSUMER)
    n_launches, n_allocs = lib.gz_emu_launch_calls() - launches, lib.gz_emu_alloc_calls() - allocs
    assert n_launches >= 8 and n_allocs >= 1 and live(lib) == base
    scans = [sdc.scan_of(d, 16)[0] for d in jpegs]
    for kind, count, fail in (("launch", n_launches, lib.gz_emu_fail_launch), ("allocation", n_allocs, lib.gz_emu_fail_alloc)):
        for n in range(count):
            canvas = dbc.BatchCanvas(2, dbc.SLOW, dbc.SLOW, "uint8", "HWC")
            out = device_output_batch(canvas.address, DTYPE_CODES["uint8"], canvas.strides, 2, CONSUMER)
            results = []
            fail(n)
            try:
                with pytest.raises(GuetzliAmdError, match="GZ_E_HIP|GZ_E_NOMEM"):
                    L.decode_scan_batch_device(scans, [0, 1], out, results=results)
            finally:
                fail(-1)
            assert live(lib) == base, f"{kind} {n} failing leaves {live(lib)} behind"
            assert all(r == {"status": "NOT_CONVERGED", "subsequences": 0, "sync_rounds": 0, "end_offset": 0} for r in results), results
            check_batch(L, host, jpegs, f"after {kind} {n}", 16, stream=CONSUMER)


# ------------------------------------------------------------------ arguments ----
def test_argument_refusals_need_no_device():
    """GZ_E_ARG from the PRODUCT library, on a machine without a GPU: the checks come before any device call."""
    from guetzli_amd import build as gzbuild
    P = Library(gzbuild.build())
    jpegs = dbc.synthetic_batches()["444_40x24"]
    other_size = dbc.synthetic_batches()["444_8x8"][0]
    other_sampling = sdc.synthetic("odd", "420", 40, 24, [np.zeros((n, 64), np.int64) for n in (15, 6, 6)], np.ones((3, 64)), "short").jpeg

    def call(members=jpegs, slots=None, n_out=None, change=None, subseqs=None, rounds=None, null=None):
        scans = [sdc.scan_of(d, (subseqs or [0] * len(members))[i], (rounds or [0] * len(members))[i])[0] for i, d in enumerate(members)]
        n = len(scans)
        arr = (capi.GzScan * max(n, 1))()
        for i, sc in enumerate(scans):
            C.memmove(C.byref(arr, i * C.sizeof(capi.GzScan)), C.byref(sc), C.sizeof(capi.GzScan))
        canvas = dbc.BatchCanvas(n_out or max(n, 1), 40, 24, "uint8", "HWC")
        out = device_output_batch(canvas.address, 0, canvas.strides, n_out or max(n, 1), 0)
        if change:
            change(out)
        res = (capi.GzScanResult * max(n, 1))()
        sl = (C.c_int * max(n, 1))(*(slots if slots is not None else range(n)))
        rc = P.lib.gz_decode_scan_batch_device(0, n, None if null == "scans" else arr, None if null == "slots" else sl,
                                               None if null == "out" else C.byref(out), None if null == "results" else res, 0)
        assert np.array_equal(canvas.raw, canvas.before)
        return rc

    assert call(members=[]) == -1                                       # n = 0
    for null in ("scans", "slots", "out", "results"):
        assert call(null=null) == -1, null
    assert call(members=jpegs[:2] + [other_size]) == -1                 # mixed w / h
    assert call(members=jpegs[:2] + [other_sampling]) == -1             # mixed sampling
    assert call(subseqs=[16, 16, 32, 16]) == -1 and call(rounds=[3, 3, 3, 4]) == -1
    assert call(subseqs=[12] * 4) == -1                                 # (check_scan's own, per scan)
    assert call(slots=[0, 1, 2, 4]) == -1 and call(slots=[0, 1, -1, 2]) == -1 and call(slots=[0, 1, 1, 2]) == -1
    assert call(slots=[0, 1, 2, 4], n_out=5) != -1                      # (in range now: it gets as far as the device)

    def overlapping(out):
        out.stride_n = out.stride_n - 3
    assert call(change=overlapping) == -1
    assert call(change=lambda o: setattr(o, "struct_size", o.struct_size - 4)) == -1
    assert call(change=lambda o: setattr(o, "dtype", 9)) == -1
    assert call(change=lambda o: setattr(o, "n", 0)) == -1
    assert call(change=lambda o: setattr(o, "stride_x", -3)) == -1


# ------------------------------------------------------------------ bounds, under the host sanitizers ----
def test_the_batched_kernels_stay_inside_their_buffers(tmp_path):
    """tests/cpp/scan_batch_bounds.cc: the batched kernels on descriptor, lane, boundary, DC and coefficient buffers malloc'ed to
    their exact sizes -- the 256 / 257 / 1-lane batch, the slow stream between neighbours, 2000 mutated streams in batches of
    8 -- built as a plain program with AddressSanitizer and UBSan.  Its own process, nothing preloaded."""
    import subprocess
    root = os.path.dirname(HERE)
    exe = str(tmp_path / "scan_batch_bounds")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-DGZ_EMU", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-w", "-I" + os.path.join(root, "tests", "emu"), "-x", "c++",
                    os.path.join(root, "tests", "cpp", "scan_batch_bounds.cc"), "-o", exe], check=True)
    out = subprocess.run([exe, sdc.GOLDEN], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "no access outside the buffers" in out.stdout


# ------------------------------------------------------------------ the driver and the Python surface ----
import fake_device  # noqa: E402
from fake_device import FakeDeviceArray  # noqa: E402


@pytest.fixture()
def emulated(monkeypatch, host):
    """guetzli_amd's module-level functions on the emulated libraries, with numpy memory for the tensors they allocate."""
    from guetzli_amd import encoder
    monkeypatch.setattr(encoder, "_default", host)
    fake_device.install(monkeypatch)


INFO_KEYS = ("path", "status", "subsequences", "sync_rounds", "end_offset")


def test_decode_batch_on_mixed_batches(emulated, L, host):
    """Eligible 4:4:4, 4:2:0 and grey images, a restart twin, a progressive twin and a stream the device hands back, in ONE
    batch: image i is decode(jpegs[i], entropy="host"), infos[i] is decode_info(jpegs[i], entropy="device")'s, and
    entropy="host" gives the same pixels."""
    import guetzli_amd
    import inspect
    assert inspect.signature(guetzli_amd.decode_batch).parameters["entropy"].default == "device"
    assert inspect.signature(guetzli_amd.decode).parameters["entropy"].default == "host"
    w, h = 40, 24
    geom_q = np.ones((3, 64))
    rng = np.random.default_rng(5)
    import entropy_domain as ed
    members = {
        "444": dbc.synthetic_batches()["444_40x24"][0],
        "420": sdc.synthetic("m420", "420", w, h, sdc._rand_blocks(ed.Geom("420", w, h), rng, 0.4, -20, 20), geom_q, "deep").jpeg,
        "grey": sdc.synthetic("mgrey", "gray", w, h, sdc._rand_blocks(ed.Geom("gray", w, h), rng, 0.4, -20, 20), geom_q, "short").jpeg,
        "444 again": dbc.synthetic_batches()["444_40x24"][1],
    }
    jpegs = list(members.values())
    got, infos = guetzli_amd.decode_batch_info(jpegs, device=0)
    assert got.array.shape == (4, h, w, 3)
    for i, data in enumerate(jpegs):
        want = guetzli_amd.decode(data, device=0, entropy="host").array
        assert np.array_equal(got.array[i], want), i
        one = guetzli_amd.decode_info(data, device=0, entropy="device")
        assert {k: infos[i][k] for k in INFO_KEYS} == {k: one[k] for k in INFO_KEYS} and infos[i]["path"] == "device", (i, infos[i], one)
    assert np.array_equal(guetzli_amd.decode_batch(jpegs, device=0, entropy="host").array, got.array)
    # one size by construction: a fixture, its twins, and mutated streams of it -- among them one the host reads and the
    # device does not decode
    name = "64x48_q90_444"
    mutated = next(s for n, k, s in sdc.mutation_sets(1000) if n == name)[:60]
    handed_back = None
    for d in mutated:
        if host.decode_jpeg_coeffs(d, "host") is not None and single(L, host, d)[0]["status"] != "DECODED":
            handed_back = d
            break
    jpegs = dbc.mixed_batch(name) + [d for d in mutated[:12] if host.decode_jpeg_coeffs(d, "host") is not None]
    if handed_back is not None:
        jpegs.append(handed_back)
    slow = dbc.slow_batch()
    canvas = np.full((len(jpegs) * 2, 48 + 5, 64 + 7, 3), 9, np.uint8)
    view = canvas[::2, 2:50, 3:67]
    got, infos = guetzli_amd.decode_batch_info(jpegs, out=FakeDeviceArray(view, strides=view.strides))
    assert got.array is view
    paths = set()
    for i, data in enumerate(jpegs):
        assert np.array_equal(view[i], guetzli_amd.decode(data, device=0, entropy="host").array), i
        one = guetzli_amd.decode_info(data, device=0, entropy="device")
        assert {k: infos[i][k] for k in INFO_KEYS} == {k: one[k] for k in INFO_KEYS}, (i, infos[i], one)
        paths.add((infos[i]["path"], infos[i]["status"]))
    assert ("device", "DECODED") in paths and ("host", None) in paths, paths
    view[...] = 9
    assert (canvas == 9).all()
    # a scan the device hands back inside a batch: NOT_CONVERGED with one round, the host's pixels
    got, infos = guetzli_amd.decode_batch_info(slow, device=0, subseq_bytes=16, max_sync_rounds=1)
    assert [(i["path"], i["status"]) for i in infos] == [("device", "DECODED"), ("host", "NOT_CONVERGED"), ("device", "DECODED")], infos
    for i, data in enumerate(slow):
        assert np.array_equal(got.array[i], guetzli_amd.decode(data, device=0).array)
    chw = guetzli_amd.decode_batch(jpegs[:3], device=0, layout="CHW", dtype="float32").array
    assert chw.shape == (3, 3, 48, 64)
    assert np.array_equal(chw, doc.emitted(view_pixels(guetzli_amd, jpegs[:3]), "float32").transpose(0, 3, 1, 2))


def view_pixels(guetzli_amd, jpegs):
    return np.stack([guetzli_amd.decode(d, device=0).array for d in jpegs])


def test_decode_batch_refusals(emulated, host):
    import guetzli_amd
    jpegs = dbc.synthetic_batches()["444_40x24"]
    with pytest.raises(ValueError, match=r"jpegs\[2\] holds 8 x 8 pixels, jpegs\[0\] 40 x 24"):
        guetzli_amd.decode_batch(jpegs[:2] + [dbc.synthetic_batches()["444_8x8"][0]], device=0)
    broken = jpegs[1][:len(jpegs[1]) // 2]   # (cut inside the scan: the device says ENDS_EARLY, the host refuses the file)
    with pytest.raises(ValueError, match=r"jpegs\[1\]"):
        guetzli_amd.decode_batch([jpegs[0], broken, jpegs[2]], device=0)
    with pytest.raises(ValueError, match=r"jpegs\[1\]"):
        guetzli_amd.decode_batch([jpegs[0], broken, jpegs[2]], device=0, entropy="host")
    with pytest.raises(ValueError, match="entropy"):
        guetzli_amd.decode_batch(jpegs, device=0, entropy="gpu")
    with pytest.raises(ValueError, match="empty"):
        guetzli_amd.decode_batch([], device=0)
    with pytest.raises(TypeError):
        guetzli_amd.decode_batch(jpegs[0], device=0)
    out = FakeDeviceArray(np.zeros((3, 24, 40, 3), np.uint8))
    with pytest.raises(ValueError, match="shape"):
        guetzli_amd.decode_batch(jpegs, out=out)


def test_a_failed_device_call_falls_back_and_says_so(emulated, L, host, capfd):
    """Through the driver: a launch of the batched call failing -> the host reads the scans, the pixels are its own, and the
    infos carry the call's error; one line on stderr for the call."""
    import guetzli_amd
    jpegs = dbc.synthetic_batches()["444_40x24"]
    want = guetzli_amd.decode_batch(jpegs, device=0, entropy="host").array
    L.lib.gz_emu_fail_launch(1)
    try:
        got, infos = guetzli_amd.decode_batch_info(jpegs, device=0)
    finally:
        L.lib.gz_emu_fail_launch(-1)
    assert np.array_equal(got.array, want)
    assert all(i["path"] == "host" and i["status"] is None and i["rc"] == -3 for i in infos), infos
    assert capfd.readouterr().err.count("batched scan decoder failed") == 1
    got, infos = guetzli_amd.decode_batch_info(jpegs, device=0)
    assert np.array_equal(got.array, want) and all(i["path"] == "device" and i["rc"] == 0 for i in infos)
