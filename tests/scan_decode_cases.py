"""The cases of the device's scan decoder (gz_decode_scan / gz_decode_scan_device, guetzli_amd.decode(entropy="device")),
shared by the emulation tests (test_scan_decode_emu.py) and the GPU tests (test_scan_decode_gpu.py).

Fixtures: the JPEGs of tests/golden/scan_decode/ (tools/make_scan_decode_fixtures.py: Pillow's libjpeg), the eligible
ones and their twins the decoder must leave to the host.  Synthetic scans: units from entropy_domain.symbolize, coded by
entropy_domain.encode under prefix codes chosen here (canonical, so that a DHT can hold them), wrapped into a whole
JPEG so that the host reader can judge them.  Mutations: single-bit flips and single-byte replacements at uniform
positions in the scan.  The judge of everything is the host reader (HostLibrary.decode_jpeg_coeffs(entropy="host"))."""
import os

import numpy as np

import entropy_domain as ed
from guetzli_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "scan_decode")
ELIGIBLE = ["64x48_q90_444", "61x43_q85_420", "96x64_q75_444_opt", "33x31_grey", "8x8_444", "8x8_420", "1x1_444", "1x1_420",
            "9x8_444", "9x8_420", "17x9_444", "17x9_420", "160x120_q95_444"]
TWINS = [n + t for n in ELIGIBLE for t in ("__progressive", "__restart", "__422") if not (t == "__422" and "grey" in n)]
MULTI_WG = "160x120_q95_444"          # at 16 bytes per lane: three workgroups of the synchronisation kernel or more
MUTATED = ["64x48_q90_444", "61x43_q85_420", "96x64_q75_444_opt"]
SUBSEQ = [16, 32, 128, 0]             # 0: the library's default
LANES = 256                           # lanes per workgroup (kScanDecLanes)
ERROR_STATUSES = ("BAD_SYMBOL", "RUN_PAST_BAND", "DC_RANGE", "COEFF_RANGE", "ENDS_EARLY")


def fixture(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
        return f.read()


# ------------------------------------------------------------------------------ a JPEG's scan as a gz_scan ----
def parse_jpeg(data):
    """The marker segments in front of the first SOS of a well-formed baseline file -> what a gz_scan needs."""
    q, dc, ac = {}, {}, {}
    pos, frame = 2, None
    while True:
        assert data[pos] == 0xff, pos
        m, n = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        seg = data[pos + 4:pos + 2 + n]
        if m == 0xdb:
            i = 0
            while i < len(seg):
                prec, tq = seg[i] >> 4, seg[i] & 15
                i += 1
                zz = [(seg[i + 2 * k] << 8) | seg[i + 2 * k + 1] for k in range(64)] if prec else list(seg[i:i + 64])
                i += 128 if prec else 64
                nat = [0] * 64
                for k in range(64):
                    nat[int(ed.NATURAL[k])] = zz[k]
                q.setdefault(tq, nat)
        elif m == 0xc4:
            i = 0
            while i < len(seg):
                tc, th = seg[i] >> 4, seg[i] & 15
                counts = list(seg[i + 1:i + 17])
                values = list(seg[i + 17:i + 17 + sum(counts)])
                i += 17 + sum(counts)
                (ac if tc else dc)[th] = (counts, values)
        elif m in (0xc0, 0xc1, 0xc2):
            h, w, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            frame = {"w": w, "h": h, "comps": [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nc)]}
        elif m == 0xda:
            ns = seg[0]
            sel = [(seg[1 + 2 * i], seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(ns)]
            assert [s[0] for s in sel] == [c[0] for c in frame["comps"]]
            nc = len(sel)
            factor = 2 if nc == 3 and frame["comps"][0][1:3] == (2, 2) else 1
            return {"w": frame["w"], "h": frame["h"], "ncomp": nc, "factor": factor, "scan_at": pos + 2 + n,
                    "dc": [dc[s[1]] for s in sel], "ac": [ac[s[2]] for s in sel], "quant": [q[c[3]] for c in frame["comps"]]}
        pos += 2 + n


def scan_of(data, subseq_bytes=0, max_sync_rounds=0):
    """(the GzScan of the file's scan, what parse_jpeg found)."""
    j = parse_jpeg(data)
    return capi.scan_spec(j["w"], j["h"], j["ncomp"], j["factor"], data[j["scan_at"]:], j["dc"], j["ac"], j["quant"], subseq_bytes,
                          max_sync_rounds), j


# ------------------------------------------------------------------------------ synthetic scans ----
def code_lengths(freq, kind):
    """Code lengths for the used symbols of one table, sorted by falling frequency.  "short": one length for all, the
    shortest that fits; "deep": the rarer half gets lengths 10 .. 16 in turns, the rarest 16 -- the decoder's slow path.
    The lengths leave room for one more code of the longest length, as ProcessDHT demands."""
    syms = sorted(freq, key=lambda s: (-freq[s], s))
    n = len(syms)
    m = 0 if kind == "short" else max(1, n // 2) if n > 1 else 0
    tail = [10 + (i % 7) for i in range(m)]
    if m:
        tail[-1] = 16
    for L in range(1, 10):
        lens = [L] * (n - m) + tail
        if sum(1 << (16 - x) for x in lens) + (1 << (16 - max(lens))) <= 65536:
            return dict(zip(syms, lens))
    raise AssertionError("no code")


def canonical(lengths):
    """{symbol: length} -> (counts[16], values, {symbol: code}): the code a DHT with these counts and values means."""
    values = sorted(lengths, key=lambda s: (lengths[s], s))
    counts = [sum(1 for s in values if lengths[s] == x) for x in range(1, 17)]
    code, k, codes = 0, 0, {}
    for x in range(1, 17):
        for _ in range(counts[x - 1]):
            codes[values[k]] = code
            code += 1
            k += 1
        code <<= 1
    return counts, values, codes


def _segment(marker, payload):
    return bytes([0xff, marker, (len(payload) + 2) >> 8, (len(payload) + 2) & 255]) + bytes(payload)


class Synthetic:
    pass


def synthetic(name, layout, w, h, blocks, q, kind):
    """blocks: per coded component [n][64] QUANTISED values (natural order) on the grid inside the image; q [3][64] <= 255.
    Returns the whole JPEG, the expected dequantised frame coefficients and the census of what the scan holds."""
    geom = ed.Geom(layout, w, h)
    q = np.asarray(q, np.int64).reshape(3, 64)
    deq = [np.asarray(b, np.int64).reshape(-1, 64) * q[c] for c, b in enumerate(blocks)]
    s = ed.symbolize(geom, deq, q)
    depth, code = np.zeros((6, 256), np.int64), np.zeros((6, 256), np.int64)
    dht, lengths_used = b"", []
    for t in range(6):
        c = t % 3
        if c >= geom.ncomp:
            continue
        hist = s.hist.reshape(6, 256)[t]
        freq = {int(v): int(hist[v]) for v in np.flatnonzero(hist)} or {0: 1}
        lens = code_lengths(freq, kind)
        counts, values, codes = canonical(lens)
        for v in lens:
            depth[t, v], code[t, v] = lens[v], codes[v]
            lengths_used.append(lens[v])
        dht += bytes([(0x10 if t >= 3 else 0) | c]) + bytes(counts) + bytes(values)
    coded = ed.encode(s, depth.reshape(2, 3, 256), code.reshape(2, 3, 256))
    dqt = b"".join(bytes([c]) + bytes(int(q[c][ed.NATURAL[k]]) for k in range(64)) for c in range(geom.ncomp))
    samp = [0x22, 0x11, 0x11] if layout == "420" else [0x11] * 3
    sof = bytes([8, h >> 8, h & 255, w >> 8, w & 255, geom.ncomp]) + b"".join(bytes([c + 1, samp[c], c]) for c in range(geom.ncomp))
    sos = bytes([geom.ncomp]) + b"".join(bytes([c + 1, (c << 4) | c]) for c in range(geom.ncomp)) + bytes([0, 63, 0])
    r = Synthetic()
    r.name = name
    r.jpeg = b"\xff\xd8" + _segment(0xdb, dqt) + _segment(0xc0, sof) + _segment(0xc4, dht) + _segment(0xda, sos) + coded.stuffed + b"\xff\xd9"
    r.scan_len = len(coded.stuffed)
    r.stuffed = coded.stuffed
    r.max_code_length = max(lengths_used)
    r.used_lengths = lengths_used
    r.census = coded.census
    r.expected = np.asarray(geom.coeff_array(deq), np.int16).reshape(-1, 64)
    return r


def _rand_blocks(geom, rng, density, lo, hi):
    out = []
    for c in range(geom.ncomp):
        n = geom.grid[c][0] * geom.grid[c][1]
        b = rng.integers(lo, hi + 1, (n, 64)) * (rng.random((n, 64)) < density)
        b[:, 0] = rng.integers(-60, 61, n)
        out.append(b)
    return out


def synthetic_cases():
    """name -> Synthetic, built once per process."""
    if _CACHE:
        return _CACHE
    rng = np.random.default_rng(2024)
    q123 = np.stack([np.full(64, 1), np.full(64, 2), np.full(64, 3)])
    qmix = np.stack([1 + (np.arange(64) % 5), 2 + (np.arange(64) % 3), np.full(64, 1)])

    def add(name, layout, w, h, make, q, kind):
        geom = ed.Geom(layout, w, h)
        _CACHE[name] = synthetic(name, layout, w, h, make(geom), q, kind)

    # codes of up to 16 bits: the slow path behind the 9-bit table
    add("deep_codes_444", "444", 40, 24, lambda g: _rand_blocks(g, rng, 0.3, -40, 40), qmix, "deep")
    add("deep_codes_420", "420", 41, 23, lambda g: _rand_blocks(g, rng, 0.3, -40, 40), qmix, "deep")
    add("deep_codes_grey", "gray", 33, 17, lambda g: _rand_blocks(g, rng, 0.5, -200, 200), qmix, "deep")

    def extremes(g):   # AC +-1023, DC differences +-2047
        out = []
        for c in range(g.ncomp):
            n = g.grid[c][0] * g.grid[c][1]
            b = np.zeros((n, 64), np.int64)
            b[:, 0] = np.where(np.arange(n) % 2 == 0, 1024, -1023)
            b[:, 1::7] = np.where((np.arange(n)[:, None] + np.arange(9)[None, :]) % 2 == 0, 1023, -1023)
            out.append(b)
        return out
    add("extremes", "444", 24, 16, extremes, q123, "short")

    def zrl(g):   # runs of 16, 32, 48 and 62 zeros: ZRL chains; coefficient 63 set: no end-of-block symbol
        out = []
        for c in range(g.ncomp):
            n = g.grid[c][0] * g.grid[c][1]
            b = np.zeros((n, 64), np.int64)
            for i in range(n):
                zz = np.zeros(64, np.int64)
                kind = i % 4
                if kind == 0:
                    zz[63] = 5 - i % 3
                elif kind == 1:
                    zz[17], zz[50], zz[63] = 1, -2, 3
                elif kind == 2:
                    zz[33] = -7
                else:
                    zz[49], zz[63] = 2, -1
                b[i][ed.NATURAL] = zz
                b[i, 0] = i
            out.append(b)
        return out
    add("zrl_chains", "444", 32, 16, zrl, q123, "deep")
    add("all_zero", "420", 33, 17, lambda g: [np.zeros((g.grid[c][0] * g.grid[c][1], 64), np.int64) for c in range(g.ncomp)], q123, "short")

    def ones(g):   # values whose extra bits are all ones: the stream is dense in 0xff bytes
        out = []
        for c in range(g.ncomp):
            n = g.grid[c][0] * g.grid[c][1]
            b = np.where(rng.random((n, 64)) < 0.8, 1023, 255)
            b[:, 0] = np.where(np.arange(n) % 2 == 0, 1023, -1024)
            out.append(b)
        return out
    add("ff_dense", "444", 24, 16, ones, q123, "short")
    return _CACHE


_CACHE = {}


def straddling_pairs(stuffed, subseq):
    """Positions of the 0xff of every stuffed pair whose 0x00 is the first byte of a subsequence."""
    a = np.frombuffer(stuffed, np.uint8)
    at = np.flatnonzero((a[:-1] == 0xff) & (a[1:] == 0))
    return at[(at + 1) % subseq == 0]


def slow_to_synchronise():
    """A stream that does NOT synchronise inside a workgroup: a grey image whose every block is "DC difference 0, end of
    block" under a two-bit DC code 00 and a one-bit end-of-block code 0 -- the stream is zeros, three bits a block.  A
    lane that starts blind at a bit that is no multiple of three reads the same zeros as valid blocks of its own phase
    and never meets the true one: the state behind a workgroup is right only once the workgroup before it was."""
    w = h = 1200
    nblocks = (w // 8) * (h // 8)
    bits = np.zeros(-(-3 * nblocks // 8) * 8, np.uint8)
    bits[3 * nblocks:] = 1
    scan = np.packbits(bits).tobytes()
    assert b"\xff" not in scan
    dqt = bytes([0]) + bytes([1] * 64)
    sof = bytes([8, h >> 8, h & 255, w >> 8, w & 255, 1, 1, 0x11, 0])
    dht = bytes([0x00, 0, 1] + [0] * 14 + [0]) + bytes([0x10, 1] + [0] * 15 + [0])
    sos = bytes([1, 1, 0x00, 0, 63, 0])
    seg = _segment
    return b"\xff\xd8" + seg(0xdb, dqt) + seg(0xc0, sof) + seg(0xc4, dht) + seg(0xda, sos) + scan + b"\xff\xd9", len(scan)


# ------------------------------------------------------------------------------ mutations ----
def mutation_sets(count=1000):
    """The six sets in the order ONE default_rng(1) runs through them -- per fixture its bit flips, then its byte
    replacements: (fixture, "bit" | "byte", [mutated JPEG ...])."""
    rng = np.random.default_rng(1)
    for name in MUTATED:
        for kind in ("bit", "byte"):
            data = fixture(name)
            at0 = parse_jpeg(data)["scan_at"]
            out = []
            for _ in range(count):
                b = bytearray(data)
                p = int(rng.integers(at0, len(data) - 2))   # (the scan: up to the EOI)
                if kind == "bit":
                    b[p] ^= 1 << int(rng.integers(0, 8))
                else:
                    b[p] = int(rng.integers(0, 256))
                out.append(bytes(b))
            yield name, kind, out


def check_mutations(L, host, streams, what):
    """The conditions every set of mutated streams is held to; returns (streams the host accepts, streams the device did
    not synchronise on) for the caller's bounds.
      - verdict, coefficients, size and metadata of the hooked reader are the plain host reader's for every stream;
      - every stream the host accepts comes back DECODED from the device, or NOT_CONVERGED;
      - every stream the device answers with one of the five error statuses is one the host refuses."""
    accepted = not_converged = 0
    for i, data in enumerate(streams):
        plain = host.decode_jpeg_coeffs(data, "host")
        got = host.decode_jpeg_coeffs(data, "device")
        assert (plain is None) == (got is None), (what, i)
        scan, _ = scan_of(data)
        status = L.decode_scan(scan)[1]["status"]
        if plain is None:   # (any status: also DECODED, where the host refuses what stands BEHIND the scan)
            continue
        # the host accepts the stream: no error status, which is the third condition read the other way round
        accepted += 1
        assert np.array_equal(got[0], plain[0]) and got[1] == plain[1] and got[3] == plain[3], (what, i, got[2])
        assert got[2]["status"] == status and status in ("DECODED", "NOT_CONVERGED"), (what, i, got[2], status)
        assert got[2]["path"] == ("device" if status == "DECODED" else "host"), (what, i, got[2])
        not_converged += status == "NOT_CONVERGED"
    return accepted, not_converged
