"""The cases of the batched device decode (gz_decode_scan_batch_device, DecodeJpegBatchToRGB, guetzli_amd.decode_batch),
shared by tests/test_decode_batch_emu.py and tests/test_decode_batch_gpu.py.  Batches are N JPEGs of ONE decoded size:

  synthetic_batches()   scan_decode_cases.synthetic() streams of one size with different contents, quantisers and code
                        families ("deep": 16-bit codes, "short"), in 4:4:4, 4:2:0 and grey, and at 8 x 8 and 1 x 1;
  lane_batch()          grey streams of 64 x 64 whose length is chosen to the bit: exactly 256 lanes, 257 lanes (a one-lane
                        second workgroup) and 1 lane at 16 bytes a lane;
  slow_batch()          scan_decode_cases.slow_to_synchronise()'s construction with blocks of 127 zero bits at 184 x 184 -- just
                        over two workgroups at 16 bytes a lane -- between two images of that size that need no round;
  mutated_batches()     the mutation sets of one fixture, which are one size by construction;
  mixed_batch()         per size the eligible fixture, its restart and progressive twins.

The judge of everything is the host reader; nothing here decodes.  scratch_bytes() restates the header's account of the
call's temporaries, for the caps that force chunks."""
import numpy as np

import entropy_domain as ed
import scan_decode_cases as sdc

LANES = sdc.LANES


# ------------------------------------------------------------------------------ grey streams coded by hand ----
# DC: the one symbol 0 (a difference of 0) under a code of dc_bits zeros.  AC: end of block '0', (run 0, size 1) '10' and
# (run 0, size 10) '110'; a coefficient is +1 ('10' '1'), -1 ('10' '0') or 512 ('110' '1000000000').  No eight ones in
# a row anywhere, so no byte is 0xff and nothing is stuffed: a stream's length is its bits, rounded up.
def grey_jpeg(w, h, blocks, dc_bits=1):
    """blocks: per block the AC values from zig-zag position 1 on, each +1, -1 or 512, at most 62 of them."""
    assert len(blocks) == ((w + 7) // 8) * ((h + 7) // 8) and dc_bits in (1, 2)
    bits = []
    for ac in blocks:
        assert len(ac) <= 62
        bits += [0] * dc_bits
        for v in ac:
            bits += {1: [1, 0, 1], -1: [1, 0, 0], 512: [1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]}[v]
        bits.append(0)
    bits += [1] * (-len(bits) % 8)
    scan = np.packbits(np.array(bits, np.uint8)).tobytes()
    assert b"\xff" not in scan
    dqt = bytes([0]) + bytes([1] * 64)
    sof = bytes([8, h >> 8, h & 255, w >> 8, w & 255, 1, 1, 0x11, 0])
    dc_counts = [1] + [0] * 15 if dc_bits == 1 else [0, 1] + [0] * 14
    dht = bytes([0x00] + dc_counts + [0]) + bytes([0x10, 1, 1, 1] + [0] * 13 + [0x00, 0x01, 0x0a])
    sos = bytes([1, 1, 0x00, 0, 63, 0])
    seg = sdc._segment
    return b"\xff\xd8" + seg(0xdb, dqt) + seg(0xc0, sof) + seg(0xc4, dht) + seg(0xda, sos) + scan + b"\xff\xd9", len(scan)


def _grey_of_length(w, h, nbytes):
    """A w x h grey stream of exactly nbytes: every block the same number of 512s, then +-1s until the bits are there."""
    n = ((w + 7) // 8) * ((h + 7) // 8)
    want = 8 * nbytes - 4                     # (some bits short of the last byte's end: the padding ones make it whole)
    big = min(45, max(0, (want // n - 2) // 13))
    blocks = [[512] * big for _ in range(n)]
    have = n * (2 + 13 * big)
    i = 0
    while have + 3 <= want:
        assert len(blocks[i % n]) < 62
        blocks[i % n].append(1 if (i // n) % 2 == 0 else -1)
        have += 3
        i += 1
    data, length = grey_jpeg(w, h, blocks)
    assert length == nbytes, (length, nbytes)
    return data


def lane_batch():
    """{"256": ..., "257": ..., "1": ...}: 64 x 64 grey JPEGs of exactly that many lanes at 16 bytes a lane."""
    if "lanes" not in _CACHE:
        one, n1 = grey_jpeg(64, 64, [[] for _ in range(64)])      # two bits a block: 16 bytes
        assert n1 == 16
        _CACHE["lanes"] = {"256": _grey_of_length(64, 64, 256 * 16 - 7), "257": _grey_of_length(64, 64, 256 * 16 + 1), "1": one}
    return _CACHE["lanes"]


def lanes_of(data, subseq=16):
    return max(1, -(-(len(data) - 2 - sdc.parse_jpeg(data)["scan_at"]) // subseq))


SLOW = 184


def slow_jpeg(w, h):
    """scan_decode_cases.slow_to_synchronise()'s construction with long blocks: DC difference 0 under the one-bit code '0',
    then 63 coefficients of -1, each the one-bit code '0' of (run 0, size 1) and the bit '0' -- 127 zero bits a block, no
    end-of-block.  A lane that starts blind reads the same zeros as blocks of its own phase and never meets the true one (both
    are periodic in 127 bits): the state behind a workgroup is right only once the workgroup before it was."""
    n = ((w + 7) // 8) * ((h + 7) // 8)
    bits = np.zeros(-(-127 * n // 8) * 8, np.uint8)
    bits[127 * n:] = 1
    scan = np.packbits(bits).tobytes()
    assert b"\xff" not in scan
    dqt = bytes([0]) + bytes([1] * 64)
    sof = bytes([8, h >> 8, h & 255, w >> 8, w & 255, 1, 1, 0x11, 0])
    dht = bytes([0x00, 1] + [0] * 15 + [0]) + bytes([0x10, 1] + [0] * 15 + [0x01])
    sos = bytes([1, 1, 0x00, 0, 63, 0])
    seg = sdc._segment
    return b"\xff\xd8" + seg(0xdb, dqt) + seg(0xc0, sof) + seg(0xc4, dht) + seg(0xda, sos) + scan + b"\xff\xd9", len(scan)


def slow_batch():
    """[quick, slow, quick]: 184 x 184 grey, 529 blocks.  slow: slow_jpeg -- just over two workgroups at 16 bytes a lane, and
    more than one round between them (the issue's 840 x 840 at three bits a block is just over ONE workgroup and settles
    in one round: not the case that was asked for); the other two: a few lanes each, one workgroup, no round."""
    if "slow" not in _CACHE:
        n = ((SLOW + 7) // 8) ** 2
        slow, length = slow_jpeg(SLOW, SLOW)
        assert 2 * 16 * LANES < length <= 2 * 16 * LANES + 16 * 16
        quick = grey_jpeg(SLOW, SLOW, [[] for _ in range(n)])[0]
        other = grey_jpeg(SLOW, SLOW, [[1, -1, 512] if i % 7 == 0 else [] for i in range(n)])[0]
        assert lanes_of(quick) <= LANES and lanes_of(other) <= LANES
        _CACHE["slow"] = [quick, slow, other]
    return _CACHE["slow"]


# ------------------------------------------------------------------------------ synthetic batches ----
def synthetic_batches():
    """name -> [JPEG ...] of one size and one sampling: contents, quantisers and code families differ."""
    if "synthetic" in _CACHE:
        return _CACHE["synthetic"]
    rng = np.random.default_rng(77)
    q123 = np.stack([np.full(64, 1), np.full(64, 2), np.full(64, 3)])
    qmix = np.stack([1 + (np.arange(64) % 5), 2 + (np.arange(64) % 3), np.full(64, 1)])
    q7 = np.stack([np.full(64, 7), 3 + (np.arange(64) % 4), np.full(64, 2)])
    out = {}
    for layout, w, h in (("444", 40, 24), ("420", 41, 23), ("gray", 33, 17), ("444", 8, 8), ("420", 8, 8), ("444", 1, 1), ("420", 1, 1)):
        geom = ed.Geom(layout, w, h)
        members = []
        for k, (kind, q, density, hi) in enumerate((("deep", qmix, 0.3, 40), ("short", q123, 0.6, 9), ("deep", q7, 0.1, 200),
                                                    ("short", qmix, 0.9, 3))):
            case = sdc.synthetic(f"{layout}_{w}x{h}_{k}", layout, w, h, sdc._rand_blocks(geom, rng, density, -hi, hi), q, kind)
            members.append(case.jpeg)
        out[f"{layout}_{w}x{h}"] = members
    _CACHE["synthetic"] = out
    return out


def mutated_batches(count, per_batch=8):
    """(fixture, kind, [batch ...]): the first `count` streams of each of scan_decode_cases' six sets in batches of
    per_batch, the unmutated fixture the first member of every batch."""
    for name, kind, streams in sdc.mutation_sets(1000):   # (the sets as the single-image tests know them, then their first ones)
        streams = streams[:count]
        yield name, kind, [[sdc.fixture(name)] + streams[i:i + per_batch - 1] for i in range(0, len(streams), per_batch - 1)]


def mixed_batch(name):
    """The eligible fixture `name`, its restart twin, its progressive twin, the fixture again."""
    return [sdc.fixture(name), sdc.fixture(name + "__restart"), sdc.fixture(name + "__progressive"), sdc.fixture(name)]


# ------------------------------------------------------------------------------ a batch's destination ----
class BatchCanvas:
    """n images of w x h x 3 inside ONE buffer pre-filled with device_output_cases' sentinel: raw (bytes), offset (the
    element that is (0, 0, 0, 0)), strides (n, y, x, c) in elements.  "HWC": contiguous images (the 16-byte stores where w
    allows them); "HWC_odd_n": an element between the images (stride_n no multiple of the vector: element by element);
    "CHW_crop_base1": planar crops inside larger planes, one element off alignment."""

    def __init__(self, n, w, h, dtype, layout):
        import device_input_cases as dic
        import device_output_cases as doc
        self.n, self.w, self.h, self.dtype, self.layout = n, w, h, dtype, layout
        self.itemsize = np.dtype(doc.STORAGE[dtype]).itemsize
        if layout in ("HWC", "HWC_odd_n"):
            sn = h * w * 3 + (1 if layout == "HWC_odd_n" else 0)
            self.strides, self.offset, total = (sn, 3 * w, 3, 1), 0, n * sn + 5
        else:
            assert layout == "CHW_crop_base1"
            cw, ch = (w + 16 + 15) // 16 * 16, h + 2
            sn = 3 * ch * cw
            self.strides, self.offset, total = (sn, cw, 1, ch * cw), 1 + cw + 16, n * sn + 1
        self.raw = dic.aligned_empty(total * self.itemsize, np.uint8, 0)
        self.raw[...] = doc.sentinel(self.raw.size)
        self.before = self.raw.copy()

    @property
    def address(self):
        return self.raw.ctypes.data + self.offset * self.itemsize

    def images_of(self, raw):
        """The [n][h][w][3] strided view of the images inside `raw`."""
        import device_output_cases as doc
        el = raw.view(doc.STORAGE[self.dtype])
        return np.lib.stride_tricks.as_strided(el[self.offset:], (self.n, self.h, self.w, 3), tuple(s * self.itemsize for s in self.strides))

    def check(self, pixels, raw=None, what=""):
        """pixels: slot -> uint8 [h][w][3], or None for an image that must be untouched.  Every byte of the buffer is
        compared: the sentinel, and the emitted image where one is expected."""
        import device_output_cases as doc
        raw = self.raw if raw is None else raw
        exp = self.before.copy()
        view = self.images_of(exp)
        for slot, rgb in pixels.items():
            if rgb is not None:
                view[slot] = doc.emitted(rgb, self.dtype)
        bad = np.flatnonzero(raw != exp)
        assert bad.size == 0, (what, self.dtype, self.layout, bad[:8], bad.size)


# ------------------------------------------------------------------------------ the scratch of a call ----
def scratch_bytes(jpegs, subseq=0):
    """include/guetzli_amd.h's account of gz_decode_scan_batch_device's temporaries for these scans as ONE chunk."""
    def a16(x):
        return (x + 15) // 16 * 16
    subseq = subseq or 64
    j0 = sdc.parse_jpeg(jpegs[0])
    w, h, f, ncomp = j0["w"], j0["h"], j0["factor"], j0["ncomp"]
    m = len(jpegs)
    upload = lanes = wgs = blocks = 0
    cols, rows = -(-w // (8 * f)), -(-h // (8 * f))
    for data in jpegs:
        end = len(data) - 2 - sdc.parse_jpeg(data)["scan_at"]      # (streams whose data end at the EOI)
        nsub = max(1, -(-end // subseq))
        nwg = -(-nsub // LANES)
        upload += a16(max(end, 1))
        lanes += nwg * LANES
        wgs += nwg
        blocks += cols * rows * (1 if ncomp == 1 else 6 if f == 2 else 3)
    tables = 6 * 512 * 2 + 6 * 18 * 4 + 6 * 17 * 4 * 2 + 6 * 4 + 6 * 256 + 3 * 64 * 4
    state = (-(-lanes // 2048) + 1) * 20 + 64
    total = a16(tables * m) + a16(72 * m) + a16(4 * wgs) + upload + 2 * a16(8 * lanes) + a16(8 * (lanes + 1)) + a16(16 * wgs) + \
        a16(4 * lanes) + a16(4 * m) + a16(state) + a16(2 * blocks) + 16 * m + a16(8 * m)
    nb, nbc = -(-w // 8) * -(-h // 8), cols * rows
    frame = (nb + 2 * nbc) * 128 + a16(3 * w * h) + (2 * (-(-w // 16) * 8) * (-(-h // 16) * 8) if f == 2 else 0)
    return total + m * frame + 1024


_CACHE = {}
