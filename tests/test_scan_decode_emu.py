"""The device's scan decoder (gz_decode_scan / gz_decode_scan_device, the reader's scan-decoder hook, decode(entropy=)) without
a GPU: the four kernels of gz_kernels_scandec.h through the CPU emulation, the host driver linked against it.  Every
comparison is for equality, and the judge is the project's host reader (HostLibrary.decode_jpeg_coeffs(entropy="host"):
ReadJpeg and DecodedCoeffs, which test_jpeg_reader.py and the fuzzer pin to the reference).  CPU only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "emu")]
import build_emu  # noqa: E402
import device_output_cases as doc  # noqa: E402
import scan_decode_cases as sdc  # noqa: E402
from guetzli_amd import capi  # noqa: E402
from guetzli_amd.capi import GuetzliAmdError, Library, device_output  # noqa: E402
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


@pytest.fixture(scope="module")
def judged(host):
    """name -> (the JPEG, the host reader's coefficients) for every fixture and synthetic scan, read once."""
    out = {}
    for name in sdc.ELIGIBLE:
        data = sdc.fixture(name)
        out[name] = (data, host.decode_jpeg_coeffs(data, "host")[0])
    for name, case in sdc.synthetic_cases().items():
        ref = host.decode_jpeg_coeffs(case.jpeg, "host")[0]
        assert np.array_equal(ref, case.expected), name   # (the host reader reads what the coder was given)
        out[name] = (case.jpeg, ref)
    return out


def live(lib):
    v = [C.c_long() for _ in range(4)]
    lib.gz_emu_live(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def output_of(dest, stream=0):
    return device_output(dest.address, DTYPE_CODES[dest.dtype], dest.strides, stream)


# ------------------------------------------------------------------ what the synthetic scans hold ----
def test_the_synthetic_scans_cover_what_they_are_for():
    cases = sdc.synthetic_cases()
    for name in ("deep_codes_444", "deep_codes_420", "deep_codes_grey", "zrl_chains"):
        # a symbol in use with a code of more than nine bits misses the first-level table: the slow path; 16 bits is the limit
        assert cases[name].max_code_length == 16 and sum(1 for x in cases[name].used_lengths if x > 9) >= 3, name
    c = cases["extremes"].census
    assert c["dc_size/11/pos"] > 0 and c["dc_size/11/neg"] > 0          # DC differences of +-2047
    assert int(np.abs(cases["extremes"].expected[: 3 * 2 * 3]).max()) >= 1023
    q = np.array([1, 2, 3]).repeat(6)[:, None]
    ac = cases["extremes"].expected[:, 1:] // q
    assert ac.max() == 1023 and ac.min() == -1023
    c = cases["zrl_chains"].census
    assert c["zrl_per_coeff/1"] > 0 and c["zrl_per_coeff/2"] > 0 and c["zrl_per_coeff/3"] > 0 and c["eob/absent"] > 0
    c = cases["all_zero"].census
    assert c["eob/alone"] == 3 * 2 * 6 and c["pad_block/right"] + c["pad_block/below"] + c["pad_block/corner"] > 0
    ff = cases["ff_dense"]
    assert ff.stuffed.count(b"\xff\x00") * 8 > len(ff.stuffed)           # an eighth of the bytes and more are 0xff
    at = sdc.straddling_pairs(ff.stuffed, 16)
    assert at.size >= 1 and all((int(a) + 1) % 16 == 0 and ff.stuffed[int(a)] == 0xff and ff.stuffed[int(a) + 1] == 0 for a in at)
    assert sdc.straddling_pairs(ff.stuffed, 32).size >= 1 and sdc.straddling_pairs(ff.stuffed, 128).size >= 1


# ------------------------------------------------------------------ coefficients and end_offset ----
@pytest.mark.parametrize("subseq", sdc.SUBSEQ)
def test_coefficients_and_end_offset_are_the_hosts(L, judged, subseq):
    """gz_decode_scan on every fixture and synthetic scan: the host reader's coefficients, and the parser continues at
    the EOI, where the host's BitReader leaves it in these files."""
    for name, (data, ref) in judged.items():
        scan, j = sdc.scan_of(data, subseq)
        co, res = L.decode_scan(scan)
        assert res["status"] == "DECODED", (name, subseq, res)
        assert np.array_equal(co, ref), (name, subseq, np.argwhere(co != ref)[:4])
        assert j["scan_at"] + res["end_offset"] == len(data) - 2, (name, subseq, res)
        assert res["subsequences"] == max(1, -(-(len(data) - 2 - j["scan_at"]) // (subseq or 64))), (name, subseq, res)


def test_the_multi_workgroup_stream_spans_three_workgroups(L, judged):
    scan, _ = sdc.scan_of(judged[sdc.MULTI_WG][0], 16)
    _, res = L.decode_scan(scan)
    assert res["subsequences"] > 2 * sdc.LANES and res["sync_rounds"] >= 1, res


# ------------------------------------------------------------------ the hooked reader ----
def test_the_hooked_reader_reads_what_the_host_reads(host, judged):
    """DecodeJpegCoeffs with the device hook: the device path for every eligible file, the host's coefficients and
    metadata; the ineligible twins -- progressive, restart interval, 4:2:2 -- take the host path and say so."""
    for name, (data, ref) in judged.items():
        plain = host.decode_jpeg_coeffs(data, "host")
        got = host.decode_jpeg_coeffs(data, "device")
        assert plain[2]["path"] == "host" and plain[2]["status"] is None
        assert got[2]["path"] == "device" and got[2]["status"] == "DECODED", (name, got[2])
        assert np.array_equal(got[0], ref) and got[1] == plain[1] and got[3] == plain[3], name
    for name in sdc.TWINS:
        data = sdc.fixture(name)
        plain, got = host.decode_jpeg_coeffs(data, "host"), host.decode_jpeg_coeffs(data, "device")
        if plain is None:   # (4:2:2: the reader accepts it, DecodeJpegToRGB has no pixels for it)
            assert got is None and name.endswith("__422"), name
            continue
        assert got[2]["path"] == "host" and got[2]["status"] is None, (name, got[2])
        assert np.array_equal(got[0], plain[0]) and got[1] == plain[1] and got[3] == plain[3], name


# ------------------------------------------------------------------ pixels, sentinels ----
PIXEL_CASES = ["64x48_q90_444", "61x43_q85_420", "33x31_grey", "17x9_420", "1x1_420", "ff_dense"]


@pytest.mark.parametrize("layout", ["HWC", "CHW_crop_base1"])
@pytest.mark.parametrize("dtype", ["uint8", "bfloat16"])
def test_pixels_go_into_the_image_and_nowhere_else(L, judged, dtype, layout):
    """gz_decode_scan_device: the pixels gz_decode_coeffs makes of the host reader's coefficients, every byte of the
    canvas outside the image untouched; with and without a consumer stream."""
    for i, name in enumerate(PIXEL_CASES):
        data, ref = judged[name]
        scan, j = sdc.scan_of(data)
        w, h = j["w"], j["h"]
        rgb = L.decode_coeffs(ref if j["factor"] == 2 else ref.reshape(3, -1, 64), w, h, j["factor"])
        dest = doc.destination(w, h, dtype, layout)
        res = L.decode_scan_device(scan, output_of(dest, CONSUMER if i % 2 else 0))
        assert res["status"] == "DECODED", (name, res)
        dest.check(rgb, what=name)


def test_a_fallback_writes_nothing(L, host, judged):
    """A scan cut short, scans with a flipped bit that the host refuses, and one that is not given its rounds: a status,
    GZ_OK, and not one byte of the canvas written."""
    data, _ = judged["64x48_q90_444"]
    at = sdc.parse_jpeg(data)["scan_at"]
    streams = [(data[:at + 400] + b"\xff\xd9", {})]
    for p in range(at + 100, at + 400, 7):
        flipped = data[:p] + bytes([data[p] ^ 0x10]) + data[p + 1:]
        if host.decode_jpeg_coeffs(flipped, "host") is None:
            streams.append((flipped, {}))
    slow, _ = sdc.slow_to_synchronise()
    streams.append((slow, {"subseq_bytes": 16, "max_sync_rounds": 1}))
    seen = []
    for stream, kw in streams:
        scan, j = sdc.scan_of(stream, **kw)
        dest = doc.destination(j["w"], j["h"], "uint8", "HWC_crop")
        res = L.decode_scan_device(scan, output_of(dest))
        seen.append(res["status"])
        assert res["status"] != "DECODED", res
        assert np.array_equal(dest.raw, dest.before), res
    assert seen[0] == "ENDS_EARLY" and seen[-1] == "NOT_CONVERGED" and len(seen) >= 4 and set(seen[1:-1]) <= set(sdc.ERROR_STATUSES), seen


# ------------------------------------------------------------------ more than one inter-workgroup round ----
def test_rounds_between_workgroups_and_not_converged(L, host):
    data, scan_len = sdc.slow_to_synchronise()
    ref = host.decode_jpeg_coeffs(data, "host")
    assert ref is not None and not ref[0].any()
    scan, j = sdc.scan_of(data, 16)
    assert scan_len > 2 * 16 * sdc.LANES          # three workgroups
    co, res = L.decode_scan(scan)
    assert res["status"] == "DECODED" and res["sync_rounds"] > 1, res
    assert np.array_equal(co, ref[0]) and j["scan_at"] + res["end_offset"] == len(data) - 2
    rounds = res["sync_rounds"]
    scan, _ = sdc.scan_of(data, 16, rounds - 1)
    co, res = L.decode_scan(scan)
    assert co is None and res["status"] == "NOT_CONVERGED" and res["sync_rounds"] == rounds - 1, res
    # ... and the decode falls back: the host's coefficients and the host's pixels
    got = host.decode_jpeg_coeffs(data, "device", subseq_bytes=16, max_sync_rounds=rounds - 1)
    assert got[2]["path"] == "host" and got[2]["status"] == "NOT_CONVERGED" and np.array_equal(got[0], ref[0])
    got = host.decode_jpeg_coeffs(data, "device", subseq_bytes=16, max_sync_rounds=rounds)
    assert got[2]["path"] == "device" and got[2]["sync_rounds"] == rounds and np.array_equal(got[0], ref[0])
    w, h = j["w"], j["h"]
    rgb = L.decode_coeffs(ref[0].reshape(3, -1, 64), w, h)
    for max_rounds, path in ((rounds - 1, "host"), (rounds, "device")):
        dest = doc.destination(w, h, "uint8", "HWC")
        info = host.decode_jpeg_device_entropy(data, dest.address, "uint8", dest.strides, size=(w, h), entropy="device",
                                               subseq_bytes=16, max_sync_rounds=max_rounds)
        assert info["path"] == path, info
        dest.check(rgb, what=path)


# ------------------------------------------------------------------ mutations ----
@pytest.fixture(scope="module")
def mutation_sets():
    return list(sdc.mutation_sets(1000))


@pytest.mark.parametrize("which", range(6))
def test_mutated_streams_get_the_hosts_verdict(L, host, mutation_sets, which):
    """One of the six sets (1000 single-bit flips or single-byte replacements at uniform positions in the scan of a
    fixture): sdc.check_mutations states the conditions."""
    name, kind, streams = mutation_sets[which]
    accepted, not_converged = sdc.check_mutations(L, host, streams, f"{name} {kind}")
    print(f"{name} {kind}: the host accepts {accepted} of {len(streams)}, {not_converged} did not synchronise")
    assert accepted >= 800 and not_converged <= 10, (name, kind, accepted, not_converged)
    # (what the host reader accepts of these sets: the figures the sets were specified with)
    assert accepted == (957, 933, 976, 953, 890, 858)[which], (name, kind, accepted)


# ------------------------------------------------------------------ failures injected ----
@pytest.mark.parametrize("entry", ["host", "device"])
def test_every_launch_and_allocation_failing_in_turn(L, judged, entry):
    """Each launch and each allocation of the call failing in turn: GZ_E_HIP / GZ_E_NOMEM, nothing written, nothing left
    allocated, and the next call is correct.  (The multi-workgroup stream at 16 bytes: every kernel, a round included.)"""
    lib = L.lib
    data, ref = judged[sdc.MULTI_WG]
    scan, j = sdc.scan_of(data, 16)
    w, h = j["w"], j["h"]
    rgb = L.decode_coeffs(ref.reshape(3, -1, 64), w, h)
    dest = doc.destination(w, h, "uint8", "HWC_crop")

    def call():
        if entry == "host":
            return L.decode_scan(scan)[0]
        assert L.decode_scan_device(scan, output_of(dest, CONSUMER))["status"] == "DECODED"
        return None

    def check(co):
        if entry == "host":
            assert np.array_equal(co, ref)
        else:
            dest.check(rgb)
            dest.raw[...] = dest.before

    base = live(lib)
    launches, allocs = lib.gz_emu_launch_calls(), lib.gz_emu_alloc_calls()
    check(call())
    n_launches, n_allocs = lib.gz_emu_launch_calls() - launches, lib.gz_emu_alloc_calls() - allocs
    assert n_launches >= (5 if entry == "host" else 7) and n_allocs >= 1 and live(lib) == base
    for n in range(n_launches):
        lib.gz_emu_fail_launch(n)
        try:
            with pytest.raises(GuetzliAmdError, match="GZ_E_HIP"):
                call()
        finally:
            lib.gz_emu_fail_launch(-1)
        assert live(lib) == base, f"launch {n} failing leaves {live(lib)} behind"
        assert np.array_equal(dest.raw, dest.before), f"launch {n} failing: the canvas was written"
        check(call())
    for n in range(n_allocs):
        lib.gz_emu_fail_alloc(n)
        try:
            with pytest.raises(GuetzliAmdError, match="GZ_E_NOMEM|GZ_E_HIP"):
                call()
        finally:
            lib.gz_emu_fail_alloc(-1)
        assert live(lib) == base, f"allocation {n} failing leaves {live(lib)} behind"
        assert np.array_equal(dest.raw, dest.before)
        check(call())


# ------------------------------------------------------------------ bounds, under the host sanitizers ----
def test_the_kernels_stay_inside_their_buffers(tmp_path):
    """tests/cpp/scan_decode_bounds.cc: the four kernels on the fixtures and on 2000 mutated streams, every buffer
    malloc'ed to its exact size, built as a plain program with AddressSanitizer and UBSan.  Its own process, nothing
    preloaded."""
    import subprocess
    root = os.path.dirname(HERE)
    exe = str(tmp_path / "scan_decode_bounds")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-DGZ_EMU", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-w", "-I" + os.path.join(root, "tests", "emu"), "-x", "c++",
                    os.path.join(root, "tests", "cpp", "scan_decode_bounds.cc"), "-o", exe], check=True)
    out = subprocess.run([exe, sdc.GOLDEN], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "no access outside the buffers" in out.stdout


def test_a_failed_device_call_falls_back_and_says_so(L, host, judged):
    """Through the driver: a launch of gz_decode_scan failing -> the host reads the scan, the coefficients are its own, and
    the entropy info tells the failed call (rc = GZ_E_HIP) from a scan that was never offered (rc = 0, no status)."""
    data, ref = judged["64x48_q90_444"]
    L.lib.gz_emu_fail_launch(1)
    try:
        got = host.decode_jpeg_coeffs(data, "device")
    finally:
        L.lib.gz_emu_fail_launch(-1)
    assert got[2]["path"] == "host" and got[2]["status"] is None and got[2]["rc"] == -3, got[2]
    assert np.array_equal(got[0], ref)
    got = host.decode_jpeg_coeffs(data, "device")
    assert got[2]["path"] == "device" and got[2]["rc"] == 0 and np.array_equal(got[0], ref)
    got = host.decode_jpeg_coeffs(sdc.fixture("64x48_q90_444__restart"), "device")
    assert got[2]["path"] == "host" and got[2]["status"] is None and got[2]["rc"] == 0


# ------------------------------------------------------------------ arguments ----
def test_argument_refusals_need_no_device():
    """GZ_E_ARG from the PRODUCT library, on a machine without a GPU: the checks come before any device call."""
    from guetzli_amd import build as gzbuild
    P = Library(gzbuild.build())
    data = sdc.fixture("64x48_q90_444")
    dest = doc.destination(64, 48, "uint8", "HWC")
    out = output_of(dest)
    res = capi.GzScanResult()
    co = np.zeros((3 * 48, 64), np.int16)

    def refused(change, **kw):
        scan, _ = sdc.scan_of(data, **kw)
        change(scan)
        assert P.lib.gz_decode_scan(0, C.byref(scan), co.ctypes.data, C.byref(res)) == -1
        assert P.lib.gz_decode_scan_device(0, C.byref(scan), C.byref(out), C.byref(res)) == -1

    refused(lambda s: setattr(s, "struct_size", s.struct_size - 4))
    for bad in (8, 12, 18, 1028, 2048, -16):
        refused(lambda s: None, subseq_bytes=bad)
    refused(lambda s: None, max_sync_rounds=-1)
    for field, bad in (("w", 0), ("h", 0), ("w", 65536), ("h", -3), ("ncomp", 2), ("ncomp", 4), ("chroma_factor", 0), ("chroma_factor", 3),
                       ("len", 2), ("len", 1 << 28), ("data", None)):
        refused(lambda s, f=field, b=bad: setattr(s, f, b))

    def grey_420(s):
        s.ncomp, s.chroma_factor = 1, 2
    refused(grey_420)

    def too_many_dc(s):          # thirteen DC symbols
        s.dc[0].counts[4] += 8
    refused(too_many_dc)

    def dc_symbol_12(s):
        s.dc[1].values[0] = 12
    refused(dc_symbol_12)

    def twice(s):
        s.ac[0].values[1] = s.ac[0].values[0]
    refused(twice)

    def complete_code(s):        # no room for one more code of the longest length
        for i in range(16):
            s.ac[2].counts[i] = 0
        s.ac[2].counts[0] = 2
    refused(complete_code)

    def zero_quantiser(s):
        s.quant[1][5] = 0
    refused(zero_quantiser)
    scan, _ = sdc.scan_of(data)
    assert P.lib.gz_decode_scan(0, C.byref(scan), None, C.byref(res)) == -1
    assert P.lib.gz_decode_scan(0, C.byref(scan), co.ctypes.data, None) == -1
    assert P.lib.gz_decode_scan_device(0, C.byref(scan), None, C.byref(res)) == -1
    bad_out = output_of(dest)
    bad_out.stride_x = 0
    assert P.lib.gz_decode_scan_device(0, C.byref(scan), C.byref(bad_out), C.byref(res)) == -1
    assert np.array_equal(dest.raw, dest.before) and not co.any()


# ------------------------------------------------------------------ the enqueue order ----
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


def test_the_four_passes_in_order_on_one_stream(L, judged):
    """The enqueue log of gz_decode_scan_device on the slow-to-synchronise stream: first-synchronise, one
    next-synchronise and ONE host read (a device-to-host copy and a wait) per round, offsets, write, DC, the final read,
    then reconstruction and emit -- all on one stream, and no other wait in between."""
    data, _ = sdc.slow_to_synchronise()
    scan, j = sdc.scan_of(data, 16)
    dest = doc.destination(j["w"], j["h"], "uint8", "HWC")
    res = {}
    log = enqueue_log(L, lambda: res.update(L.decode_scan_device(scan, output_of(dest))))
    assert res["status"] == "DECODED" and res["sync_rounds"] >= 2
    streams = {ln.split()[-1] for ln in log if ln.split()[0] in ("launch", "memcpy", "memset", "stream_sync")}
    assert streams == {"s0"}, log
    steps = [ln.split()[1] if ln.startswith("launch") else " ".join(ln.split()[:2]) if ln.startswith("memcpy") else ln.split()[0] for ln in log]
    kernels = [s for s in steps if s.startswith("k_")]
    r = res["sync_rounds"]
    assert kernels[:1 + r + 3] == ["k_scandec_sync_first"] + ["k_scandec_sync_next"] * r + ["k_scan_offsets", "k_scandec_write", "k_scandec_dc"], kernels
    assert "k_emit_rgb" in kernels[-1], kernels
    # the host's reads: behind every round's launch a 4-byte copy and a wait; then none until the verdict's 8 bytes
    first = steps.index("k_scandec_sync_first")
    dc = steps.index("k_scandec_dc")
    between = [s for s in steps[first + 1:dc + 1] if not s.startswith("k_")]
    assert between == ["memcpy d2h", "stream_sync"] * r, between
    assert steps[dc + 1:dc + 3] == ["memcpy d2h", "stream_sync"], steps[dc:]
    d2h = [ln for ln in log if ln.startswith("memcpy d2h")]
    assert [ln.split()[2] for ln in d2h] == ["4"] * r + ["8"], d2h
    assert steps.count("stream_sync") == r + 2    # ... and the wait for the pixels


# ------------------------------------------------------------------ the Python surface ----
import fake_device  # noqa: E402
from fake_device import FakeDeviceArray  # noqa: E402


@pytest.fixture()
def emulated(monkeypatch, host):
    """guetzli_amd's module-level functions on the emulated libraries, with numpy memory for the tensors they allocate."""
    from guetzli_amd import encoder
    monkeypatch.setattr(encoder, "_default", host)
    fake_device.install(monkeypatch)


def test_decode_and_decode_info(emulated, judged):
    """decode(entropy="device") returns decode(entropy="host")'s pixels, into a fresh image and into a crop of the
    caller's; decode_info says which path ran; the default is the host; an ineligible stream falls back silently."""
    import guetzli_amd
    import inspect
    assert inspect.signature(guetzli_amd.decode).parameters["entropy"].default == "host"
    for name in ("64x48_q90_444", "61x43_q85_420", "33x31_grey", "64x48_q90_444__restart", "61x43_q85_420__progressive"):
        data = judged[name][0] if name in judged else sdc.fixture(name)
        eligible = "__" not in name
        want = guetzli_amd.decode(data, device=0).array
        assert np.array_equal(want, guetzli_amd.decode(data, device="host"))
        assert np.array_equal(guetzli_amd.decode(data, device=0, entropy="device").array, want), name
        h, w = want.shape[:2]
        canvas = np.full((h + 9, w + 13, 3), 7, np.uint8)
        view = canvas[4:4 + h, 6:6 + w]
        info = guetzli_amd.decode_info(data, out=FakeDeviceArray(view, strides=view.strides))
        assert info["path"] == ("device" if eligible else "host") and info["status"] == ("DECODED" if eligible else None), (name, info)
        assert info["decoded"].array is view and np.array_equal(view, want)
        view[...] = 7
        assert (canvas == 7).all()
        info = guetzli_amd.decode_info(data, entropy="host", device=0)
        assert info["path"] == "host" and info["status"] is None and np.array_equal(info["decoded"].array, want)
        if eligible:
            info = guetzli_amd.decode_info(data, device=0, subseq_bytes=16)
            assert info["subsequences"] == -(-(len(data) - 2 - sdc.parse_jpeg(data)["scan_at"]) // 16) and info["end_offset"] > 0
    with pytest.raises(ValueError, match="entropy"):
        guetzli_amd.decode(sdc.fixture("8x8_444"), entropy="gpu")
    with pytest.raises(ValueError, match="entropy"):
        guetzli_amd.decode(sdc.fixture("8x8_444"), device="host", entropy="device")
