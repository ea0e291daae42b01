"""JPEG input read by the device's scan decoder on the MI355X: gz_decode_scan_input, the host driver with the decoder
behind its reader, process_jpeg(entropy="device").  The cases are those of tests/test_jpeg_input_device_emu.py
(tests/jpeg_input_device_cases.py); here the lanes are the device's own.  Every comparison is for equality, and the judge
is the project's host reader and its host-mode encode.  The mutated streams are the first 100 of one set of the CPU
file, from the same generator: they have passed the emulation and the sanitizer program by then.  Nothing here reads a
file outside the repository tree."""
import pytest

import jpeg_input_device_cases as jic
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


def stream_of(name):
    if name in jic.FIXTURES:
        return jic.fixture(name)
    if name in jic.padded_cases():
        return jic.padded_cases()[name][0].jpeg
    if name in sdc.synthetic_cases():
        return sdc.synthetic_cases()[name].jpeg
    return sdc.fixture(name)


SCANS = [(n, 0) for n in jic.FIXTURES] + [("17x9_420", 0), ("9x8_420", 0), ("33x31_grey", 0), (sdc.MULTI_WG, 16), ("deep_codes_420", 0),
                                          ("ff_dense", 0), ("ff_dense", 16), ("extremes_in_padding", 0), ("extremes_in_padding", 16)]


@pytest.mark.parametrize("name,subseq", SCANS, ids=[f"{n}-{s}" for n, s in SCANS])
def test_the_entry_returns_the_readers_own_result(L, host, name, subseq):
    """Coefficients per component, MCU padding included, end_offset and large_coeff against the host reader's dump."""
    data = stream_of(name)
    dump, _ = host.read_jpeg_dump(data, "host")
    res = jic.check_scan_input(L, dump, data, subseq, name)
    if name == sdc.MULTI_WG:
        assert res["subsequences"] > 2 * sdc.LANES and res["sync_rounds"] == 1, res   # three workgroups


ENCODES = ["40x40_420", "40x40_444", "160x120_q95_444", "17x9_420"]


@pytest.mark.parametrize("name", ENCODES)
def test_encodes_are_the_host_modes(host, name):
    """Bytes and trace of process_jpeg(entropy="device") against entropy="host"."""
    data = stream_of(name)
    want = host.process_jpeg(data, want_trace=True)
    jpg, info = host.process_jpeg_info(data, want_trace=True, entropy="device")
    assert info["input"]["path"] == "device" and info["input"]["status"] == "DECODED" and info["input"]["rc"] == 0, info["input"]
    assert info["trace"] == want[1] and jpg == want[0]


def test_the_top_level_function_and_two_twins(host):
    import guetzli_amd
    data = stream_of("17x9_420")
    want = host.process_jpeg(data)[0]
    jpg, info = guetzli_amd.process_jpeg(data, entropy="device")
    assert jpg == want and info["input"]["path"] == "device", info["input"]
    jpg, info = guetzli_amd.process_jpeg(data)
    assert jpg == want and info["input"]["path"] == "host" and info["input"]["status"] is None, info["input"]
    for twin in ("17x9_420__restart", "64x48_q90_444__progressive"):
        data = sdc.fixture(twin)
        jpg, info = guetzli_amd.process_jpeg(data, entropy="device")
        assert info["input"]["path"] == "host" and info["input"]["status"] is None and info["input"]["rc"] == 0, (twin, info["input"])
        assert jpg == host.process_jpeg(data)[0], twin


@pytest.mark.parametrize("name", ["large_dc_in_padding", "large_ac_in_padding", "exactly_4096_in_padding"])
def test_the_padding_blocks_are_judged_alike(host, name):
    """|c q| > 4096 in a padding block alone: refused in both modes; c q == 4096 there: the same bytes in both."""
    case, refused = jic.padded_cases()[name]
    dump, info = host.read_jpeg_dump(case.jpeg, "device")
    assert info["path"] == "device" and dump == host.read_jpeg_dump(case.jpeg, "host")[0] and jic.sanity_refuses(dump) == refused
    outcome = {}
    for entropy in ("host", "device"):
        try:
            jpg, i = host.process_jpeg_info(case.jpeg, entropy=entropy, want_trace=True)
            outcome[entropy] = (jpg, i["trace"])
            assert i["input"]["path"] == entropy, i["input"]
        except RuntimeError:
            outcome[entropy] = None
    assert outcome["device"] == outcome["host"] and (outcome["host"] is None) == refused


def test_mutated_streams_get_the_hosts_verdict(host):
    """The first 100 streams of the first set, through the reader only, under the CPU file's conditions."""
    name, kind, streams = next(iter(sdc.mutation_sets(100)))
    accepted = jic.check_mutations(host, streams, f"{name} {kind}")
    print(f"{name} {kind}: the host accepts {accepted} of {len(streams)}")
    assert accepted >= 80, accepted
