"""The device's scan decoder on the MI355X: gz_decode_scan / gz_decode_scan_device, the host driver with the decoder behind
its reader, guetzli_amd.decode(entropy="device") and decode_info.  The cases are those of tests/test_scan_decode_emu.py
(tests/scan_decode_cases.py); here the lanes are the device's own, 64 to a wavefront, each on its own bit stream.  Every
comparison is for equality, and the judge is the project's host reader.  The mutated streams are the first 300 of each
set of the CPU file, from the same generator: they have passed the emulation and the sanitizer program by then."""
import numpy as np
import pytest

import device_output_cases as doc
import images
import scan_decode_cases as sdc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def L(torch):   # (torch first, as in the other GPU files: it finds the device before the library opens it)
    import guetzli_amd
    return guetzli_amd.load()


@pytest.fixture(scope="module")
def host(torch):
    import guetzli_amd
    return guetzli_amd.load_host()


@pytest.fixture(scope="module")
def judged(host):
    """name -> (the JPEG, the host reader's coefficients) for every fixture and synthetic scan, read once."""
    out = {}
    for name in sdc.ELIGIBLE:
        data = sdc.fixture(name)
        out[name] = (data, host.decode_jpeg_coeffs(data, "host")[0])
    for name, case in sdc.synthetic_cases().items():
        ref = host.decode_jpeg_coeffs(case.jpeg, "host")[0]
        assert np.array_equal(ref, case.expected), name
        out[name] = (case.jpeg, ref)
    return out


class OnDevice:
    """A doc.Destination whose buffer, sentinel included, lives on the GPU."""

    def __init__(self, torch, dest):
        self.dest = dest
        self.t = torch.from_numpy(dest.raw).cuda()

    @property
    def address(self):
        return self.t.data_ptr() + self.dest.offset * self.dest.itemsize

    def output(self, stream=0):
        from guetzli_amd.capi import device_output
        from guetzli_amd.encoder import DTYPE_CODES
        return device_output(self.address, DTYPE_CODES[self.dest.dtype], self.dest.strides, stream)

    def check(self, rgb, what=""):
        self.dest.check(rgb, raw=self.t.cpu().numpy(), what=what)

    def untouched(self):
        return np.array_equal(self.t.cpu().numpy(), self.dest.before)


@pytest.mark.parametrize("subseq", sdc.SUBSEQ)
def test_coefficients_and_end_offset_are_the_hosts(L, judged, subseq):
    """Every fixture and synthetic scan -- codes of 16 bits, +-1023 and +-2047, ZRL chains, blocks without an end-of-block,
    all-zero blocks, stuffed pairs across subsequence boundaries -- at the four subsequence sizes."""
    for name, (data, ref) in judged.items():
        scan, j = sdc.scan_of(data, subseq)
        co, res = L.decode_scan(scan)
        assert res["status"] == "DECODED", (name, subseq, res)
        assert np.array_equal(co, ref), (name, subseq, np.argwhere(co != ref)[:4])
        assert j["scan_at"] + res["end_offset"] == len(data) - 2, (name, subseq, res)


def test_straddling_pairs_and_long_codes(L, judged):
    """The two cases by name, with what makes them what they are asserted here too."""
    ff = sdc.synthetic_cases()["ff_dense"]
    for subseq in (16, 32, 128):
        at = sdc.straddling_pairs(ff.stuffed, subseq)
        assert at.size >= 1 and all((int(a) + 1) % subseq == 0 for a in at)
        co, res = L.decode_scan(sdc.scan_of(ff.jpeg, subseq)[0])
        assert res["status"] == "DECODED" and np.array_equal(co, judged["ff_dense"][1])
    for name in ("deep_codes_444", "deep_codes_420", "deep_codes_grey"):
        case = sdc.synthetic_cases()[name]
        assert case.max_code_length == 16 and sum(1 for x in case.used_lengths if x > 9) >= 3
        co, res = L.decode_scan(sdc.scan_of(case.jpeg)[0])
        assert res["status"] == "DECODED" and np.array_equal(co, judged[name][1])


def test_rounds_between_workgroups(torch, L, host, judged):
    """The multi-workgroup fixture spans three workgroups at 16 bytes a lane; the stream that does not synchronise inside
    a workgroup (scan_decode_cases.slow_to_synchronise) takes the rounds the emulation counts, and one fewer is
    NOT_CONVERGED with nothing written."""
    data, ref = judged[sdc.MULTI_WG]
    co, res = L.decode_scan(sdc.scan_of(data, 16)[0])
    assert res["subsequences"] > 2 * sdc.LANES and res["sync_rounds"] == 1 and np.array_equal(co, ref), res
    slow, _ = sdc.slow_to_synchronise()
    ref = host.decode_jpeg_coeffs(slow, "host")[0]
    scan, j = sdc.scan_of(slow, 16)
    co, res = L.decode_scan(scan)
    # (two, as in the emulation: the second round finds the last workgroup's exit state unchanged -- the padding ones at the
    # end of the data had led its wrong phase to the right state -- while it puts the lanes in front of it right)
    assert res["status"] == "DECODED" and res["sync_rounds"] == 2 and np.array_equal(co, ref), res
    assert j["scan_at"] + res["end_offset"] == len(slow) - 2
    co, res = L.decode_scan(sdc.scan_of(slow, 16, 1)[0])
    assert co is None and res["status"] == "NOT_CONVERGED" and res["sync_rounds"] == 1, res
    got = host.decode_jpeg_coeffs(slow, "device", subseq_bytes=16, max_sync_rounds=1)
    assert got[2]["path"] == "host" and got[2]["status"] == "NOT_CONVERGED" and np.array_equal(got[0], ref)
    d = OnDevice(torch, doc.destination(j["w"], j["h"], "uint8", "HWC_crop"))
    res = L.decode_scan_device(sdc.scan_of(slow, 16, 1)[0], d.output())
    assert res["status"] == "NOT_CONVERGED" and d.untouched(), res
    res = L.decode_scan_device(scan, d.output())
    assert res["status"] == "DECODED", res
    d.check(L.decode_coeffs(ref.reshape(3, -1, 64), j["w"], j["h"]), what="slow")


def test_the_hooked_reader_and_its_twins(host, judged):
    for name, (data, ref) in judged.items():
        got = host.decode_jpeg_coeffs(data, "device")
        assert got[2]["path"] == "device" and got[2]["status"] == "DECODED" and np.array_equal(got[0], ref), (name, got[2])
    for name in sdc.TWINS:
        data = sdc.fixture(name)
        plain, got = host.decode_jpeg_coeffs(data, "host"), host.decode_jpeg_coeffs(data, "device")
        assert (plain is None) == (got is None), name
        if plain is not None:
            assert got[2]["path"] == "host" and got[2]["status"] is None and np.array_equal(got[0], plain[0]), (name, got[2])


@pytest.mark.parametrize("layout", ["HWC", "CHW_crop_base1"])
@pytest.mark.parametrize("dtype", ["uint8", "bfloat16"])
def test_decode_device_against_decode_host_in_sentinel_canvases(torch, judged, dtype, layout):
    """guetzli_amd.decode(entropy="device") against decode(entropy="host") into canvases on the GPU, with and without a
    consumer stream: the same pixels, nothing outside the image; decode_info says which path ran."""
    import guetzli_amd
    s = torch.cuda.Stream()
    for i, name in enumerate(["64x48_q90_444", "61x43_q85_420", "33x31_grey", "17x9_420", "1x1_420", "ff_dense",
                              "64x48_q90_444__progressive", "61x43_q85_420__restart"]):
        data = judged[name][0] if name in judged else sdc.fixture(name)
        want = guetzli_amd.decode(data, entropy="host").cpu().numpy()
        h, w = want.shape[:2]
        stream = s.cuda_stream if i % 2 else 0
        torch.cuda.synchronize()
        d = OnDevice(torch, doc.destination(w, h, dtype, layout))
        guetzli_amd.decode(data, out=view_of(torch, d, layout), layout=layout[:3], stream=stream, entropy="device")
        with torch.cuda.stream(s):
            d.check(want, what=name)
        torch.cuda.synchronize()
        d = OnDevice(torch, doc.destination(w, h, dtype, layout))
        info = guetzli_amd.decode_info(data, out=view_of(torch, d, layout), layout=layout[:3], stream=stream, entropy="device")
        assert info["path"] == ("host" if "__" in name else "device") and info["status"] == (None if "__" in name else "DECODED"), (name, info)
        with torch.cuda.stream(s):
            d.check(want, what=name)


def view_of(torch, on_device, layout):
    """The canvas's image as a strided torch view: what decode(out=) fills in place."""
    d = on_device.dest
    el = on_device.t.view({"uint8": torch.uint8, "bfloat16": torch.bfloat16}[d.dtype])
    sy, sx, sc = d.strides
    if layout.startswith("CHW"):
        return torch.as_strided(el, (3, d.h, d.w), (sc, sy, sx), d.offset)
    return torch.as_strided(el, (d.h, d.w, 3), (sy, sx, sc), d.offset)


def test_process_then_both_decodes(torch):
    """process(images.crop(64, 48, ...), quality=95): the library's own output is an eligible scan, and both decodes of
    it give the pixels process(decoded=True) gives."""
    import guetzli_amd
    rgb = images.crop(64, 48, 120, 80)
    jpeg, info = guetzli_amd.process(rgb, quality=95, decoded=True)
    a = guetzli_amd.decode(jpeg, entropy="host")
    di = guetzli_amd.decode_info(jpeg, entropy="device")
    assert di["path"] == "device" and di["status"] == "DECODED", di
    assert torch.equal(a, di["decoded"]) and torch.equal(a, info["decoded"])
    assert torch.equal(guetzli_amd.decode(jpeg, entropy="device"), a)


@pytest.mark.parametrize("which", range(6))
def test_mutated_streams_get_the_hosts_verdict(L, host, which):
    """300 of each of the six sets, under the CPU file's conditions."""
    name, kind, streams = mutation_sets()[which]
    streams = streams[:300]
    accepted, not_converged = sdc.check_mutations(L, host, streams, f"{name} {kind}")
    print(f"{name} {kind}: the host accepts {accepted} of {len(streams)}, {not_converged} did not synchronise")
    assert accepted >= 240 and not_converged <= 3, (name, kind, accepted, not_converged)


_SETS = []


def mutation_sets():
    if not _SETS:
        _SETS.extend(sdc.mutation_sets(1000))
    return _SETS
