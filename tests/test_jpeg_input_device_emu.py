"""JPEG input read by the device's scan decoder (gz_decode_scan_input, the reader hook of Process(..., EntropyOptions),
process_jpeg(entropy="device")) without a GPU: passes 3 and 4 of gz_kernels_scandec.h in their input mode through the CPU
emulation, the host driver linked against it.  Every comparison is for equality.  The judges are the project's host
reader (HostLibrary.read_jpeg_dump(entropy="host"), which test_jpeg_reader.py and the fuzzer pin to the reference) and,
where oracle/_ref is built, the unmodified reference's ref_read_jpeg dump and ref_process_jpeg.  CPU only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "emu")]
import build_emu  # noqa: E402
import jpeg_input_device_cases as jic  # noqa: E402
import scan_decode_cases as sdc  # noqa: E402
from checkers import ref  # noqa: E402
from guetzli_amd import capi  # noqa: E402
from guetzli_amd.capi import Library  # noqa: E402


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
    """name -> (the JPEG, the host reader's dump) for every stream the device takes, read once."""
    out = {}
    for name, data in jic.eligible_streams():
        dump, info = host.read_jpeg_dump(data, "host")
        assert dump is not None and info["path"] == "host" and info["status"] is None, name
        out[name] = (data, dump)
    return out


def live(lib):
    v = [C.c_long() for _ in range(4)]
    lib.gz_emu_live(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def ref_dump(data):
    f = ref.lib.ref_read_jpeg
    f.restype, f.argtypes = C.c_long, [C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    buf = np.frombuffer(data, np.uint8)
    out = np.zeros(1 << 22, np.uint8)
    n = f(buf.ctypes.data, len(data), out.ctypes.data, out.size)
    return None if n < 0 else out[:n].tobytes()


# ------------------------------------------------------------------ the padded streams are what they are for ----
def test_the_padded_streams_hold_what_they_were_given(judged):
    """The coder of jpeg_input_device_cases.py against the host reader: every block of the padded grids comes back, and
    what CheckJpegSanity minds lies in padding blocks alone."""
    for name, (case, refused) in jic.padded_cases().items():
        coeffs, quant = jic.dump_components(judged[name][1])
        for c in range(3):
            assert np.array_equal(coeffs[c], case.grids[c]), (name, c)
        assert jic.sanity_refuses(judged[name][1]) == refused, name
        inside = [coeffs[0][:3, :3], coeffs[1], coeffs[2]]     # 24 x 24: the luma grid is 3 x 3, chroma has no padding
        assert all(int(np.abs(b.astype(np.int64) * q).max()) < 4096 for b, q in zip(inside, quant)), name
    c = jic.padded_cases()["exactly_4096_in_padding"][0]
    prod = np.abs(c.grids[0].astype(np.int64) * c.q[0])
    assert int(prod.max()) == 4096 and int((prod == 4096).sum()) == 4
    c = jic.padded_cases()["extremes_in_padding"][0]
    pad = np.array([c.grids[0][y, x] for y, x in jic.PAD_ONLY])
    assert pad[:, 1:].max() == 1023 and pad[:, 1:].min() == -1023 and int(np.abs(c.grids[0][:3, :3, 1:]).max()) < 1023
    assert list(c.grids[0][3, :, 0]) == [1024, -1023, -1023, 1024]
    # the fixtures' padding has content of its own: libjpeg's edge replication, right, below and corner
    luma = jic.dump_components(judged["40x40_420"][1])[0][0]
    assert luma.shape == (6, 6, 64) and luma[:5, 5].any() and luma[5, :5].any() and luma[5, 5].any()
    luma = jic.dump_components(judged["64x40_420"][1])[0][0]
    assert luma.shape == (6, 8, 64) and luma[5].any()
    assert jic.dump_components(judged["72x40_420"][1])[0][0].shape == (6, 10, 64)


# ------------------------------------------------------------------ gz_decode_scan_input ----
@pytest.mark.parametrize("subseq", sdc.SUBSEQ)
def test_the_entry_returns_the_readers_own_result(L, judged, subseq):
    """Coefficients per component equal to the host reader's dump, MCU padding included; end_offset as gz_decode_scan's;
    large_coeff the host loop's verdict."""
    for name, (data, dump) in judged.items():
        res = jic.check_scan_input(L, dump, data, subseq, name)
        scan, j = sdc.scan_of(data, subseq)
        if name in sdc.ELIGIBLE or name in sdc.synthetic_cases():   # (the decode entry refuses a product that leaves int16)
            assert res["end_offset"] == L.decode_scan(scan)[1]["end_offset"], name
        assert res["subsequences"] == max(1, -(-(len(data) - 2 - j["scan_at"]) // (subseq or 64))), (name, subseq, res)


def test_no_coefficient_range_refusal_in_input_mode(L, host):
    """A product that leaves int16 refuses a decode and not a read: quantisers of 255 under +-1023."""
    rng = np.random.default_rng(5)
    g = jic._quiet_grids(rng)
    g[0][0, 0, 1] = 1023
    case = jic.padded_420("wide_product", jic.W, jic.H, g, np.full((3, 64), 255))
    scan, _ = sdc.scan_of(case.jpeg)
    assert L.decode_scan(scan)[1]["status"] == "COEFF_RANGE"
    dump, _ = host.read_jpeg_dump(case.jpeg, "host")
    jic.check_scan_input(L, dump, case.jpeg, 0, "wide_product")
    assert L.decode_scan_input(scan)[1] is True


# ------------------------------------------------------------------ the hooked reader ----
def test_the_hooked_reader_dumps_what_the_host_dumps(host, judged):
    for name, (data, dump) in judged.items():
        got, info = host.read_jpeg_dump(data, "device")
        assert info["path"] == "device" and info["status"] == "DECODED" and info["rc"] == 0, (name, info)
        assert got == dump, name
        if ref is not None:
            assert got == ref_dump(data), name
    for name in sdc.TWINS:
        data = sdc.fixture(name)
        plain, _ = host.read_jpeg_dump(data, "host")
        got, info = host.read_jpeg_dump(data, "device")
        assert plain is not None and got == plain, name
        assert info["path"] == "host" and info["status"] is None and info["rc"] == 0, (name, info)


def test_not_converged_falls_back(host):
    data, _ = sdc.slow_to_synchronise()
    plain, _ = host.read_jpeg_dump(data, "host")
    got, info = host.read_jpeg_dump(data, "device", subseq_bytes=16, max_sync_rounds=1)
    assert got == plain and info["path"] == "host" and info["status"] == "NOT_CONVERGED" and info["sync_rounds"] == 1, info
    got, info = host.read_jpeg_dump(data, "device", subseq_bytes=16)
    assert got == plain and info["path"] == "device" and info["sync_rounds"] >= 2, info


# ------------------------------------------------------------------ whole encodes ----
ENCODES = [("40x40_420", {}), ("40x40_444", {}), ("64x48_q90_444", {}), ("17x9_420", {}),
           ("40x40_420", {"clear_metadata": False}), ("17x9_420", {"clear_metadata": False}), ("40x40_444", {"try_420": True})]


@pytest.mark.parametrize("name,kw", ENCODES, ids=[n + "".join("-" + k for k in kw) for n, kw in ENCODES])
def test_encodes_are_the_host_modes(host, judged, name, kw):
    """Bytes AND trace of entropy="device" equal those of entropy="host" -- and the reference's, where it is built."""
    data = judged[name][0] + (b"tail!" if kw.get("clear_metadata") is False else b"")
    want = host.process_jpeg(data, want_trace=True, **kw)
    jpg, info = host.process_jpeg_info(data, want_trace=True, entropy="device", **kw)
    assert info["input"]["path"] == "device" and info["input"]["status"] == "DECODED", info["input"]
    assert info["trace"] == want[1] and jpg == want[0]
    if name == "17x9_420":   # (... and process_jpeg's own form of the call)
        assert host.process_jpeg(data, want_trace=True, entropy="device", **kw) == want
    if ref is not None and "try_420" not in kw:
        exp = ref.process_jpeg(data, ref._butteraugli_score_for_quality(95.0), clear_metadata=kw.get("clear_metadata", True), want_trace=True)
        assert (jpg, info["trace"]) == exp


def test_the_default_is_the_host(host, judged):
    import inspect
    import guetzli_amd
    from guetzli_amd.encoder import HostLibrary
    for fn in (HostLibrary.process_jpeg, HostLibrary.process_jpeg_info, HostLibrary.read_jpeg_dump, guetzli_amd.process_jpeg):
        assert inspect.signature(fn).parameters["entropy"].default == "host"
    assert "process_jpeg" in guetzli_amd.__all__
    jpg, info = host.process_jpeg_info(judged["17x9_420"][0])
    assert info["input"] == {"path": "host", "status": None, "subsequences": 0, "sync_rounds": 0, "end_offset": 0, "rc": 0}
    with pytest.raises(ValueError, match="entropy"):
        host.process_jpeg(judged["17x9_420"][0], entropy="gpu")


def test_the_top_level_function(monkeypatch, host, judged):
    import guetzli_amd
    from guetzli_amd import encoder
    monkeypatch.setattr(encoder, "_default", host)
    data = judged["17x9_420"][0]
    want = host.process_jpeg(data)[0]
    for entropy, path in (("host", "host"), ("device", "device")):
        jpg, info = guetzli_amd.process_jpeg(data, entropy=entropy)
        assert jpg == want and info["input"]["path"] == path, info["input"]
    jpg, info = guetzli_amd.process_jpeg(sdc.fixture("17x9_420__restart"), 95.0, "device")
    assert info["input"]["path"] == "host" and jpg == host.process_jpeg(sdc.fixture("17x9_420__restart"))[0]


# ------------------------------------------------------------------ CheckJpegSanity in the padding ----
def test_the_padding_blocks_are_judged_alike(host, judged, capfd):
    for name, (case, refused) in jic.padded_cases().items():
        outcome = {}
        for entropy in ("host", "device"):
            capfd.readouterr()
            try:
                jpg, info = host.process_jpeg_info(case.jpeg, entropy=entropy, want_trace=True)
                outcome[entropy] = (jpg, info["trace"], "")
            except RuntimeError:
                outcome[entropy] = (None, None, capfd.readouterr().err)
        assert outcome["device"] == outcome["host"], name
        assert (outcome["host"][0] is None) == refused, name
        if refused:
            assert "unexpectedly large coefficient values" in outcome["host"][2], outcome["host"][2]
        assert host.read_jpeg_dump(case.jpeg, "device")[1]["path"] == "device", name


# ------------------------------------------------------------------ mutations ----
@pytest.fixture(scope="module")
def mutation_sets():
    return list(sdc.mutation_sets(1000))


@pytest.mark.parametrize("which", range(6))
def test_mutated_streams_get_the_hosts_verdict(host, mutation_sets, which):
    """One of scan_decode's six sets through the reader only: jic.check_mutations states the conditions.  The host accepts
    858 .. 976 of each thousand, so that nothing here can pass on refusals alone."""
    name, kind, streams = mutation_sets[which]
    accepted = jic.check_mutations(host, streams, f"{name} {kind}")
    print(f"{name} {kind}: the host accepts {accepted} of {len(streams)}")
    assert accepted >= 800, (name, kind, accepted)


# ------------------------------------------------------------------ failures injected ----
def test_every_launch_and_allocation_failing_in_turn(L, host, judged):
    """Each launch and each allocation of the device's read failing in turn: the encode falls back, its bytes are the host
    mode's, info["input"]["rc"] names the failure, nothing is left allocated.  (The multi-workgroup stream at 16 bytes --
    every kernel, a round included -- cut to 17 x 9 pixels' worth of work behind the read: the too-small path.)"""
    lib = L.lib
    data = judged[sdc.MULTI_WG][0]
    plain = judged[sdc.MULTI_WG][1]

    def read():
        return host.read_jpeg_dump(data, "device", subseq_bytes=16)

    base = live(lib)
    launches, allocs = lib.gz_emu_launch_calls(), lib.gz_emu_alloc_calls()
    got, info = read()
    n_launches, n_allocs = lib.gz_emu_launch_calls() - launches, lib.gz_emu_alloc_calls() - allocs
    assert got == plain and info["path"] == "device" and info["sync_rounds"] >= 1 and n_launches >= 5 and n_allocs >= 1 and live(lib) == base
    for kind, count, fail, rcs in (("launch", n_launches, lib.gz_emu_fail_launch, (-3,)), ("allocation", n_allocs, lib.gz_emu_fail_alloc, (-3, -5))):
        for n in range(count):
            fail(n)
            try:
                got, info = read()
            finally:
                fail(-1)
            assert got == plain, f"{kind} {n} failing: another dump"
            assert info["path"] == "host" and info["status"] is None and info["rc"] in rcs, (kind, n, info)
            assert live(lib) == base, f"{kind} {n} failing leaves {live(lib)} behind"
    got, info = read()
    assert got == plain and info["path"] == "device" and info["rc"] == 0
    # ... and through a whole encode: the first launch, the last launch and the first allocation
    small = judged["17x9_420"][0]
    want = host.process_jpeg(small, want_trace=True)
    launches = lib.gz_emu_launch_calls()
    assert host.process_jpeg(small, want_trace=True, entropy="device") == want
    n_launches = lib.gz_emu_launch_calls() - launches
    for fail, n, rcs in ((lib.gz_emu_fail_launch, 0, (-3,)), (lib.gz_emu_fail_launch, n_launches - 1, (-3,)), (lib.gz_emu_fail_alloc, 0, (-3, -5))):
        fail(n)
        try:
            jpg, info = host.process_jpeg_info(small, want_trace=True, entropy="device")
        finally:
            fail(-1)
        assert (jpg, info["trace"]) == want and info["input"]["path"] == "host" and info["input"]["rc"] in rcs, info["input"]
        assert live(lib) == base


# ------------------------------------------------------------------ bounds, under the host sanitizers ----
def test_the_input_mode_stays_inside_its_buffers(tmp_path):
    """tests/cpp/scan_input_bounds.cc: the passes with the input mode behind them on the fixtures, the padded streams and
    2000 mutated streams, the destination malloc'ed to exactly total * 64 elements, built as a plain program with
    AddressSanitizer and UBSan.  Its own process, nothing preloaded."""
    import subprocess
    root = os.path.dirname(HERE)
    exe = str(tmp_path / "scan_input_bounds")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-DGZ_EMU", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-w", "-I" + os.path.join(root, "tests", "emu"), "-x", "c++",
                    os.path.join(root, "tests", "cpp", "scan_input_bounds.cc"), "-o", exe], check=True)
    padded = tmp_path / "padded"
    padded.mkdir()
    for name, (case, _) in jic.padded_cases().items():
        (padded / (name + ".jpg")).write_bytes(case.jpeg)
    out = subprocess.run([exe, sdc.GOLDEN, jic.GOLDEN, str(padded)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "no access outside the buffers" in out.stdout


# ------------------------------------------------------------------ arguments ----
def test_argument_refusals_need_no_device():
    """GZ_E_ARG from the PRODUCT library, on a machine without a GPU: the checks come before any device call."""
    from guetzli_amd import build as gzbuild
    P = Library(gzbuild.build())
    data = jic.fixture("40x40_420")
    res, large = capi.GzScanResult(), C.c_int(-1)
    co = np.zeros((6 * 9, 64), np.int16)

    def call(scan, coeffs=co.ctypes.data, flag=C.byref(large), result=C.byref(res)):
        return P.lib.gz_decode_scan_input(0, None if scan is None else C.byref(scan), coeffs, flag, result)

    def refused(change, **kw):
        scan, _ = sdc.scan_of(data, **kw)
        change(scan)
        assert call(scan) == -1

    refused(lambda s: setattr(s, "struct_size", s.struct_size - 4))
    for bad in (8, 12, 18, 1028, 2048, -16):
        refused(lambda s: None, subseq_bytes=bad)
    refused(lambda s: None, max_sync_rounds=-1)
    for field, bad in (("w", 0), ("h", 0), ("w", 65536), ("h", -3), ("ncomp", 2), ("ncomp", 4), ("chroma_factor", 0), ("chroma_factor", 3),
                       ("len", 2), ("len", 1 << 28), ("data", None)):
        refused(lambda s, f=field, b=bad: setattr(s, f, b))

    def zero_quantiser(s):
        s.quant[1][5] = 0
    refused(zero_quantiser)

    def dc_symbol_12(s):
        s.dc[1].values[0] = 12
    refused(dc_symbol_12)
    scan, _ = sdc.scan_of(data)
    assert call(None) == -1
    assert call(scan, coeffs=None) == -1
    assert call(scan, flag=None) == -1
    assert call(scan, result=None) == -1
    assert not co.any() and large.value == -1


# ------------------------------------------------------------------ the enqueue order ----
def test_the_passes_of_one_call(L):
    """The enqueue log of gz_decode_scan_input on the slow-to-synchronise stream: the passes of gz_decode_scan with the
    input kernels in the places of passes 3 and 4, all on one stream; the host reads one word a round, then the verdict's
    12 bytes (error, end, large-coefficient word), then the coefficients: total * 128 bytes."""
    data, _ = sdc.slow_to_synchronise()
    scan, j = sdc.scan_of(data, 16)
    L.lib.gz_emu_enqueue_log_start()
    try:
        comps, large, res = L.decode_scan_input(scan)
    finally:
        L.lib.gz_emu_enqueue_log_stop()
    n = L.lib.gz_emu_enqueue_log_fetch(None, 0)
    buf = C.create_string_buffer(n + 1)
    L.lib.gz_emu_enqueue_log_fetch(buf, n)
    log = buf.raw[:n].decode().splitlines()
    assert res["status"] == "DECODED" and res["sync_rounds"] >= 2 and large is False and not comps[0].any()
    assert {ln.split()[-1] for ln in log if ln.split()[0] in ("launch", "memcpy", "memset", "stream_sync")} == {"s0"}, log
    steps = [ln.split()[1] if ln.startswith("launch") else " ".join(ln.split()[:2]) if ln.startswith("memcpy") else ln.split()[0] for ln in log]
    r = res["sync_rounds"]
    assert [s for s in steps if s.startswith("k_")] == ["k_scandec_sync_first"] + ["k_scandec_sync_next"] * r + \
        ["k_scan_offsets", "k_scandec_write_input", "k_scandec_dc_input"], steps
    d2h = [ln.split()[2] for ln in log if ln.startswith("memcpy d2h")]
    assert d2h == ["4"] * r + ["12", str(150 * 150 * 128)], d2h
    assert steps.count("stream_sync") == r + 2
