"""The batched device decode on the MI355X: gz_decode_scan_batch_device, DecodeJpegBatchToRGB, guetzli_amd.decode_batch.  The
cases are those of tests/test_decode_batch_emu.py (tests/decode_batch_cases.py); here the lanes are the device's own and
the workgroups of a launch run side by side.  Every comparison is for equality: a batch member's result is the single
call's for the same scan, its pixels gz_decode_coeffs' of the host reader's coefficients, decode_batch's image i
decode(jpegs[i], entropy="host").  The mutated streams have passed the emulation and the sanitizer program by then."""
import itertools

import numpy as np
import pytest

import decode_batch_cases as dbc
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


_SINGLE = {}


def single(L, host, data, subseq=0, rounds=0):
    """(the single call's result, the pixels gz_decode_coeffs makes of the host reader's coefficients or None), once per stream."""
    key = (data, subseq, rounds)
    if key not in _SINGLE:
        scan, j = sdc.scan_of(data, subseq, rounds)
        co, res = L.decode_scan(scan)
        rgb = None
        if res["status"] == "DECODED":
            ref = host.decode_jpeg_coeffs(data, "host")
            co = ref[0] if ref is not None else co   # (the host refuses what stands BEHIND a scan the device decoded)
            rgb = L.decode_coeffs(co if j["factor"] == 2 else co.reshape(3, -1, 64), j["w"], j["h"], j["factor"])
        _SINGLE[key] = (res, rgb)
    return _SINGLE[key]


def check_batch(torch, L, host, jpegs, what, subseq=0, rounds=0, dtype="uint8", layout="HWC", stream=None, scratch=0, slots=None, n_out=None):
    from guetzli_amd.capi import device_output_batch
    from guetzli_amd.encoder import DTYPE_CODES
    scans = [sdc.scan_of(d, subseq, rounds)[0] for d in jpegs]
    j = sdc.parse_jpeg(jpegs[0])
    n_out = n_out or len(jpegs)
    slots = slots or list(range(len(jpegs)))
    canvas = dbc.BatchCanvas(n_out, j["w"], j["h"], dtype, layout)
    torch.cuda.synchronize()
    t = torch.from_numpy(canvas.raw).cuda()
    out = device_output_batch(t.data_ptr() + canvas.offset * canvas.itemsize, DTYPE_CODES[dtype], canvas.strides, n_out,
                              stream.cuda_stream if stream is not None else 0)
    res = L.decode_scan_batch_device(scans, slots, out, scratch_bytes=scratch)
    want = [single(L, host, d, subseq, rounds) for d in jpegs]
    assert res == [w[0] for w in want], (what, subseq, res, [w[0] for w in want])
    if stream is not None:   # read back on the consumer's stream, without a synchronise
        with torch.cuda.stream(stream):
            raw = t.cpu().numpy()
    else:
        raw = t.cpu().numpy()
    canvas.check({slots[i]: w[1] for i, w in enumerate(want)}, raw=raw, what=what)
    return res


@pytest.mark.parametrize("subseq", [16, 0])
def test_every_member_is_its_single_call(torch, L, host, subseq):
    s = torch.cuda.Stream()
    layouts = itertools.cycle([("uint8", "HWC"), ("bfloat16", "CHW_crop_base1"), ("float32", "HWC_odd_n"), ("uint16", "HWC")])
    for i, (name, jpegs) in enumerate(dbc.synthetic_batches().items()):
        dtype, layout = next(layouts)
        check_batch(torch, L, host, jpegs, name, subseq, dtype=dtype, layout=layout, stream=s if i % 2 else None)
        check_batch(torch, L, host, jpegs[2:3], name + " alone", subseq)
    lanes = dbc.lane_batch()
    for order in itertools.permutations(["256", "257", "1"]):
        res = check_batch(torch, L, host, [lanes[k] for k in order], order, subseq)
        if subseq == 16:
            assert [r["subsequences"] for r in res] == [int(k) for k in order]
            assert [r["sync_rounds"] for r in res] == [1 if k == "257" else 0 for k in order]
    check_batch(torch, L, host, dbc.synthetic_batches()["420_41x23"], "slots", subseq, slots=[5, 0, 3, 2], n_out=7, layout="CHW_crop_base1")


def test_images_converge_in_different_rounds(torch, L, host):
    jpegs = dbc.slow_batch()
    res = check_batch(torch, L, host, jpegs, "slow", 16)
    assert [r["sync_rounds"] for r in res] == [0, 2, 0] and res[1]["subsequences"] > 2 * dbc.LANES, res
    res = check_batch(torch, L, host, jpegs, "slow, one round", 16, 1)
    assert [r["status"] for r in res] == ["DECODED", "NOT_CONVERGED", "DECODED"] and [r["sync_rounds"] for r in res] == [0, 1, 0], res
    res = check_batch(torch, L, host, [jpegs[1], jpegs[0], jpegs[1]], "slow first and last", 16)
    assert [r["sync_rounds"] for r in res] == [2, 0, 2], res


@pytest.mark.parametrize("per_chunk", [1, 2])
def test_chunks_give_the_same_results(torch, L, host, per_chunk):
    lanes = dbc.lane_batch()
    jpegs = [lanes["257"], lanes["256"], lanes["1"], lanes["257"], lanes["256"]]
    check_batch(torch, L, host, jpegs, f"chunks of {per_chunk}", 16, scratch=dbc.scratch_bytes([lanes["257"]] * per_chunk, 16), layout="HWC_odd_n")


@pytest.mark.parametrize("which", range(6))
def test_mutated_streams_in_batches(torch, L, host, which):
    """The first 300 streams of each mutation set in batches of 8 with the unmutated fixture: every member's status is its
    single-call status, images whose status is not DECODED are untouched, the others exact."""
    name, kind, batches = mutation_batches()[which]
    statuses = {}
    for i, b in enumerate(batches):
        for r in check_batch(torch, L, host, b, (name, kind, i)):
            statuses[r["status"]] = statuses.get(r["status"], 0) + 1
    print(name, kind, statuses)
    assert statuses.get("DECODED", 0) >= 240 and sum(v for k, v in statuses.items() if k in sdc.ERROR_STATUSES) >= 1, statuses


_SETS = []


def mutation_batches():
    if not _SETS:
        _SETS.extend(dbc.mutated_batches(300))
    return _SETS


@pytest.mark.parametrize("layout", ["HWC", "CHW_crop"])
@pytest.mark.parametrize("dtype", ["uint8", "bfloat16"])
def test_decode_batch_against_decode_host(torch, host, dtype, layout):
    """guetzli_amd.decode_batch of a mixed batch -- the fixture, its restart and progressive twins, mutated streams the host
    reads -- into a view inside a larger tensor, with and without a consumer stream: image i is decode(jpegs[i],
    entropy="host"), read back on that stream without a synchronise; what surrounds the view is untouched; infos[i] is
    decode_info's."""
    import guetzli_amd
    name = "64x48_q90_444"
    mutated = next(s for n, k, s in sdc.mutation_sets(1000) if n == name)[:12]
    jpegs = dbc.mixed_batch(name) + [d for d in mutated if host.decode_jpeg_coeffs(d, "host") is not None]
    n, w, h = len(jpegs), 64, 48
    want = torch.stack([guetzli_amd.decode(d, entropy="host") for d in jpegs])
    el = getattr(torch, dtype)
    s = torch.cuda.Stream()
    for stream in (None, s):
        torch.cuda.synchronize()
        if layout == "HWC":
            canvas = torch.full((2 * n, h + 4, w + 16, 3), 7, dtype=el, device="cuda")
            view = canvas[::2, 1:1 + h, 16:16 + w]
        else:
            canvas = torch.full((n, 3, h + 4, w + 16), 7, dtype=el, device="cuda")
            view = canvas[:, :, 2:2 + h, 16:16 + w]
        got, infos = guetzli_amd.decode_batch_info(jpegs, out=view, layout=layout[:3], stream=stream.cuda_stream if stream else None)
        with torch.cuda.stream(stream or torch.cuda.current_stream()):
            pixels = view if layout == "HWC" else view.permute(0, 2, 3, 1)
            exp = doc.emitted(want.cpu().numpy(), dtype)
            exp = torch.from_numpy(exp if dtype == "uint8" else exp.view(np.int16)).cuda()
            same = torch.equal(pixels.contiguous().view(torch.uint8 if dtype == "uint8" else torch.int16), exp)
            view[...] = 7
            clean = bool((canvas == 7).all())
        assert same and clean, (dtype, layout, stream)
        for i, d in enumerate(jpegs):
            one = guetzli_amd.decode_info(d, entropy="device")
            assert all(infos[i][k] == one[k] for k in ("path", "status", "subsequences", "sync_rounds", "end_offset")), (i, infos[i], one)
        assert {i["path"] for i in infos} == {"device", "host"}


def test_process_outputs_as_one_batch(torch):
    """process() outputs of one crop at three qualities as one batch: decode() of each, and then
    butteraugli_batch(reference, decode_batch(...)), whose distances are the loop's."""
    import guetzli_amd
    rgb = images.crop(64, 48, 120, 80)
    jpegs = [guetzli_amd.process(rgb, quality=q) for q in (84, 90, 95)]
    jpegs = [j[0] if isinstance(j, tuple) else j for j in jpegs]
    got, infos = guetzli_amd.decode_batch_info(jpegs)
    assert all(i["path"] == "device" and i["status"] == "DECODED" for i in infos), infos
    singles = [guetzli_amd.decode(j) for j in jpegs]
    for i in range(3):
        assert torch.equal(got[i], singles[i]), i
    ref = torch.from_numpy(np.ascontiguousarray(rgb)).cuda()
    d = guetzli_amd.butteraugli_batch(ref, got)
    loop = [float(guetzli_amd.butteraugli(ref, s)) for s in singles]
    assert [float(x) for x in d.cpu()] == loop, (d, loop)
