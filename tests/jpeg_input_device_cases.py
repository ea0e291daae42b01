"""The cases of JPEG input read by the device's scan decoder (gz_decode_scan_input, the reader hook of
Process(..., EntropyOptions), process_jpeg(entropy="device")), shared by the emulation tests
(test_jpeg_input_device_emu.py) and the GPU tests (test_jpeg_input_device_gpu.py).

What is new against scan_decode_cases.py (whose fixtures, synthetic scans, twins and mutation sets are used as they
are) is the MCU padding: this path stores the reader's own result, on grids padded to whole MCUs.  The fixtures of
tests/golden/jpeg_input_device/ (tools/make_jpeg_input_fixtures.py) have padding that libjpeg filled by edge
replication; the synthetic 4:2:0 streams here are given block by block on their PADDED grids -- entropy_domain.symbolize
pads as a writer does, so they have a small coder of their own -- and put what CheckJpegSanity looks for, and the
extreme values of the code, into padding blocks alone.  The judge of everything is the host reader's dump
(HostLibrary.read_jpeg_dump(entropy="host"), the format of host/reader_dump.h)."""
import os
import struct

import numpy as np

import entropy_domain as ed
import scan_decode_cases as sdc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "jpeg_input_device")
FIXTURES = ["40x40_420", "72x40_420", "64x40_420", "40x40_444"]


def fixture(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
        return f.read()


# ------------------------------------------------------------------------------ the reader's dump ----
def dump_components(dump):
    """The canonical dump -> (per component its quantised coefficients int16 [height_in_blocks][width_in_blocks][64],
    per component its quantisers int [64]).  The layout is reader_dump.h's."""
    at = [0]

    def i32():
        v = struct.unpack_from("<i", dump, at[0])[0]
        at[0] += 4
        return v
    i32(), i32()
    comps = []
    for _ in range(i32()):
        _id, _hs, _vs, qi, wb, hb = (i32() for _ in range(6))
        comps.append((qi, wb, hb))
    quant = []
    for _ in range(i32()):
        i32(), i32()
        quant.append([i32() for _ in range(64)])
    def skip():
        n = i32()
        at[0] += n
    for _ in range(2):            # APPn, COM
        for _ in range(i32()):
            skip()
    skip()                        # the tail
    coeffs = []
    for _, wb, hb in comps:
        n = wb * hb * 64
        coeffs.append(np.frombuffer(dump, np.int16, n, at[0]).reshape(hb, wb, 64))
        at[0] += 2 * n
    assert at[0] == len(dump)
    return coeffs, [np.array(quant[qi]) for qi, _, _ in comps]


def sanity_refuses(dump):
    """CheckJpegSanity over a dump: |coefficient * quantiser| > 4096 anywhere, the padding included."""
    coeffs, quant = dump_components(dump)
    return any(int(np.abs(c.astype(np.int64) * q).max()) > 4096 for c, q in zip(coeffs, quant))


# ------------------------------------------------------------------------------ a coder for padded grids ----
def _category(v):
    return int(abs(int(v))).bit_length()


def _extra(v, size):
    return int(v) if v >= 0 else int(v) + (1 << size) - 1


def _block_symbols(zz, diff):
    """One block as [(is_ac, symbol, extra bits, how many)]: T.81 F.1.2, zz in zig-zag order."""
    out = [(0, _category(diff), _extra(diff, _category(diff)), _category(diff))]
    run = 0
    last = max([k for k in range(1, 64) if zz[k]], default=0)
    for k in range(1, last + 1):
        if zz[k] == 0:
            run += 1
            continue
        while run > 15:
            out.append((1, 0xf0, 0, 0))
            run -= 16
        size = _category(zz[k])
        out.append((1, (run << 4) | size, _extra(zz[k], size), size))
        run = 0
    if last < 63:
        out.append((1, 0x00, 0, 0))
    return out


class Padded:
    pass


def padded_420(name, w, h, grids, q, kind="short"):
    """grids: [luma [2 rows][2 cols][64], cb [rows][cols][64], cr likewise], QUANTISED values in natural order on the
    grids padded to whole MCUs (rows, cols: the MCUs of a w x h image); q [3][64] <= 255.  Returns the whole JPEG."""
    cols, rows = -(-w // 16), -(-h // 16)
    grids = [np.asarray(g, np.int64) for g in grids]
    assert grids[0].shape == (2 * rows, 2 * cols, 64) and grids[1].shape == grids[2].shape == (rows, cols, 64)
    q = np.asarray(q, np.int64).reshape(3, 64)
    units, last = [], [0, 0, 0]
    for my in range(rows):
        for mx in range(cols):
            for c, y, x in [(0, 2 * my + (u >> 1), 2 * mx + (u & 1)) for u in range(4)] + [(1, my, mx), (2, my, mx)]:
                zz = grids[c][y, x][ed.NATURAL]
                units.append((c, _block_symbols(zz, int(zz[0]) - last[c])))
                last[c] = int(zz[0])
    freq = [{} for _ in range(6)]
    for c, syms in units:
        for is_ac, sym, _, _ in syms:
            f = freq[3 * is_ac + c]
            f[sym] = f.get(sym, 0) + 1
    dht, codes = b"", []
    for t in range(6):
        lens = sdc.code_lengths(freq[t] or {0: 1}, kind)
        counts, values, code = sdc.canonical(lens)
        codes.append({s: (code[s], lens[s]) for s in lens})
        dht += bytes([(0x10 if t >= 3 else 0) | t % 3]) + bytes(counts) + bytes(values)
    bits = []
    for c, syms in units:
        for is_ac, sym, extra, n in syms:
            code, length = codes[3 * is_ac + c][sym]
            bits.append((code, length))
            if n:
                bits.append((extra, n))
    acc, nacc, raw = 0, 0, bytearray()
    for v, n in bits:
        acc, nacc = (acc << n) | v, nacc + n
        while nacc >= 8:
            raw.append((acc >> (nacc - 8)) & 255)
            nacc -= 8
        acc &= (1 << nacc) - 1
    if nacc:
        raw.append(((acc << (8 - nacc)) | ((1 << (8 - nacc)) - 1)) & 255)
    stuffed = bytes(raw).replace(b"\xff", b"\xff\x00")
    dqt = b"".join(bytes([c]) + bytes(int(q[c][ed.NATURAL[k]]) for k in range(64)) for c in range(3))
    sof = bytes([8, h >> 8, h & 255, w >> 8, w & 255, 3]) + b"".join(bytes([c + 1, [0x22, 0x11, 0x11][c], c]) for c in range(3))
    sos = bytes([3]) + b"".join(bytes([c + 1, (c << 4) | c]) for c in range(3)) + bytes([0, 63, 0])
    seg = sdc._segment
    r = Padded()
    r.name = name
    r.jpeg = b"\xff\xd8" + seg(0xe0, b"JFIF\0\1\1\0\0\1\0\1\0\0") + seg(0xdb, dqt) + seg(0xc0, sof) + seg(0xc4, dht) + seg(0xda, sos) + \
        stuffed + b"\xff\xd9"
    r.grids = [g.astype(np.int16) for g in grids]
    r.q = q
    return r


W = H = 24                       # a 3 x 3 luma grid in a padded one of 4 x 4; under 32 pixels: the input is re-written
PAD_LUMA = [(3, 0), (1, 3), (3, 3)]   # (y, x): padding below, to the right, in the corner
PAD_ONLY = [(y, x) for y in range(4) for x in range(4) if y == 3 or x == 3]


def _quiet_grids(rng):
    """Small values everywhere, the padding included: nothing CheckJpegSanity minds under quantisers of 128."""
    grids = []
    for shape in ((4, 4, 64), (2, 2, 64), (2, 2, 64)):
        g = rng.integers(-3, 4, shape) * (rng.random(shape) < 0.2)
        g[..., 0] = rng.integers(-20, 21, shape[:2])
        grids.append(g)
    return grids


def padded_cases():
    """name -> (Padded, whether CheckJpegSanity refuses it), built once per process."""
    if _CACHE:
        return _CACHE
    rng = np.random.default_rng(77)
    q128 = np.full((3, 64), 128)
    q1 = np.ones((3, 64), np.int64)

    def add(name, grids, q, refused, kind="short"):
        _CACHE[name] = (padded_420(name, W, H, grids, q, kind), refused)

    g = _quiet_grids(rng)          # 33 * 128 = 4224 > 4096, in the corner block's DC alone
    g[0][3, 3, 0] = 33
    add("large_dc_in_padding", g, q128, True)
    g = _quiet_grids(rng)          # ... and in one AC coefficient of the block to the right
    g[0][1, 3, 9] = -33
    add("large_ac_in_padding", g, q128, True)
    g = _quiet_grids(rng)          # 32 * 128 = 4096: passes, DC and AC, both signs
    g[0][3, 3, 0], g[0][3, 0, 0], g[0][1, 3, 9], g[0][3, 3, 63] = 32, -32, -32, 32
    add("exactly_4096_in_padding", g, q128, False)
    g = _quiet_grids(rng)          # the code's extremes where only this path stores them: AC +-1023, DC differences +-2047
    for i, (y, x) in enumerate(PAD_ONLY):
        g[0][y, x, 1::7] = np.where((i + np.arange(9)) % 2 == 0, 1023, -1023)
    g[0][..., 0] = 0
    g[0][3, :, 0] = [1024, -1023, -1023, 1024]    # (an MCU's units 2 and 3 follow each other in scan order: -2047, +2047)
    add("extremes_in_padding", g, q1, False, "deep")
    return _CACHE


_CACHE = {}


# ------------------------------------------------------------------------------ what every stream is held to ----
def eligible_streams():
    """(name, JPEG) of every stream the device takes: scan_decode's fixtures and synthetic scans, the new fixtures, the
    padded streams."""
    for name in sdc.ELIGIBLE:
        yield name, sdc.fixture(name)
    for name, case in sdc.synthetic_cases().items():
        yield name, case.jpeg
    for name in FIXTURES:
        yield name, fixture(name)
    for name, (case, _) in padded_cases().items():
        yield name, case.jpeg


def check_scan_input(L, host_dump, data, subseq=0, what=""):
    """gz_decode_scan_input of the stream's scan against the host reader's dump of the stream: the coefficients per
    component, the end offset (the EOI, where the host's BitReader leaves these files), the sanity verdict."""
    scan, j = sdc.scan_of(data, subseq)
    comps, large, res = L.decode_scan_input(scan)
    assert res["status"] == "DECODED", (what, subseq, res)
    want, _ = dump_components(host_dump)
    assert len(comps) == len(want), what
    for c, (got, ref) in enumerate(zip(comps, want)):
        assert got.shape == ref.shape and np.array_equal(got, ref), (what, subseq, c, np.argwhere(got != ref)[:4])
    assert j["scan_at"] + res["end_offset"] == len(data) - 2, (what, subseq, res)
    assert large == sanity_refuses(host_dump), (what, subseq, large)
    return res


def check_mutations(host, streams, what):
    """Mutated streams through the reader only.  For every stream the device-mode dump or refusal is the host's; every
    stream the host accepts came from the device, or from a NOT_CONVERGED fallback; every device error status belongs to
    a stream the host refuses.  Returns how many the host accepts."""
    accepted = 0
    for i, data in enumerate(streams):
        plain, _ = host.read_jpeg_dump(data, "host")
        got, info = host.read_jpeg_dump(data, "device")
        assert (plain is None) == (got is None), (what, i, info)
        assert got == plain, (what, i, info)
        assert info["rc"] == 0, (what, i, info)
        if plain is not None:
            accepted += 1
            assert (info["path"], info["status"]) in (("device", "DECODED"), ("host", "NOT_CONVERGED")), (what, i, info)
        if info["status"] in sdc.ERROR_STATUSES:
            assert plain is None and info["path"] == "host", (what, i, info)
    return accepted
