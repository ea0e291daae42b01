"""Synthetic coefficient families, code tables and a plain reference coder for the device scan coder
(guetzli_amd/csrc/gz_kernels_entropy.h).

The reference coder restates, in numpy and from the reference's text alone, what the reference does between a frame's
coefficients and its scan bytes:
  OutputImage::SaveToJpegData   output_image.cc:348-407   quantised value = coefficient / q (C++ `/`), the padding blocks
  BuildDCHistograms             jpeg_data_writer.cc:234-256
  BuildACHistograms             jpeg_data_writer.cc:258-266 (UpdateACHistogramForDCTBlock)
  EncodeDCTBlockSequential      jpeg_data_writer.cc:455-500
  EncodeScan                    jpeg_data_writer.cc:502-536
  BitWriter                     jpeg_bit_writer.h:31-109  (MSB first, 0x00 after every 0xFF, 1-padding to the byte)
It shares nothing with the kernels or with guetzli_amd/host.  tests/test_entropy_domain.py pins it to the host writer
and to the reference on the optimal codes; after that it judges the device coder under ARBITRARY (depth, code) tables,
which no real writer produces.

Domain.  BuildDCHistograms takes abs() of the DC difference in `int`, EncodeDCTBlockSequential wraps it to coeff_t
(int16): the two disagree once a DC difference leaves int16, and -32768 has size 16, for which no symbol exists.  The
domain therefore stops at quantised values of +-16383 (DC differences within +-32766, sizes up to 15; a code of 16 bits
plus its extra bits is at most 31 bits).  Code lengths above 16 are out of scope: nothing here produces them and
check_prefix_code refuses them.
"""
import functools
import zlib

import numpy as np

# kJPEGNaturalOrder, jpeg_data.h:62-73: natural index of zig-zag position k
NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
                    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

STAGE_BITS = 8192            # k_jpeg_emit stages an MCU whose span is at most this many bits
SCAN_TILE = 2048             # values per tile of k_scan_offsets
MCU_PER_WAVE, MCU_WAVES = 4, 4

# The shapes of the GPU tests: (layout, w, h).  444: 1, 3, 5, 6, 15, 16, 17 MCUs; 96; 2072 (two scan tiles); 4160 (the
# statistics kernel's second grid-stride trip).  420: one luma block (three padding blocks); luma grid 11 x 7 (odd on
# both axes); 17 x 2; 56 x 37.  (48 x 8 is the one shape with two MCUs in the last wavefront.)
SHAPES = [("444", 8, 8), ("444", 24, 8), ("444", 40, 8), ("444", 48, 8), ("444", 120, 8), ("444", 128, 8),
          ("444", 136, 8), ("444", 93, 59), ("444", 448, 296), ("444", 520, 512),
          ("420", 8, 8), ("420", 85, 53), ("420", 129, 9), ("420", 448, 296),
          ("gray", 93, 59), ("gray", 448, 296)]


class Geom:
    """The frame as the JPEG sees it: per component the grid of real blocks and its blocks per MCU along each axis."""

    def __init__(self, layout, w, h):
        assert layout in ("444", "420", "gray")
        self.layout, self.w, self.h = layout, w, h
        self.bw, self.bh = (w + 7) // 8, (h + 7) // 8
        self.cbw, self.cbh = (w + 15) // 16, (h + 15) // 16
        self.nb, self.nbc = self.bw * self.bh, self.cbw * self.cbh
        if layout == "420":
            self.grid = [(self.bw, self.bh), (self.cbw, self.cbh), (self.cbw, self.cbh)]
            self.samp = [2, 1, 1]
            self.mcu_cols, self.mcu_rows = self.cbw, self.cbh
        else:
            self.grid = [(self.bw, self.bh)] * (1 if layout == "gray" else 3)
            self.samp = [1] * len(self.grid)
            self.mcu_cols, self.mcu_rows = self.bw, self.bh
        self.ncomp = len(self.grid)
        self.nmcu = self.mcu_cols * self.mcu_rows
        self.upm = sum(s * s for s in self.samp)
        self.factor = 2 if layout == "420" else 1
        # blocks of the coefficient array handed to gz_set_coeffs / write_jpeg (a grey frame is a 4:4:4 one whose chroma
        # components are entirely zero)
        self.array_blocks = [self.nb, self.nbc, self.nbc] if layout == "420" else [self.nb] * 3

    def coeff_array(self, blocks):
        """blocks: per coded component [n][64] int16, natural order -> the array of the frame layout."""
        out = [np.zeros((n, 64), np.int16) for n in self.array_blocks]
        for c, b in enumerate(blocks):
            out[c][:] = b
        if self.layout == "420":
            return np.ascontiguousarray(np.concatenate(out))
        return np.ascontiguousarray(np.stack(out))


def _size(mag):
    """Log2Floor(mag) + 1, 0 for 0."""
    mag = np.asarray(mag, np.int64)
    out = np.zeros(mag.shape, np.int64)
    m = mag.copy()
    while (m > 0).any():
        out += m > 0
        m >>= 1
    return out


class Symbols:
    """What the writer emits for one frame, before any code table: the units in stream order."""


def symbolize(geom, blocks, q):
    """blocks: per coded component [n][64] dequantised coefficients (natural order); q: [3][64].  Returns the units of
    the scan in stream order, the histograms and the table-independent census."""
    q = np.asarray(q, np.int64).reshape(3, 64)
    census = {}
    # ---- SaveToJpegData: quantise (C++ `/` truncates towards zero), pad every component to whole MCUs
    padded = []
    for c in range(geom.ncomp):
        rw, rh = geom.grid[c]
        co = np.asarray(blocks[c], np.int64).reshape(rh, rw, 64)
        qv = np.sign(co) * (np.abs(co) // q[c])
        pw, ph = geom.mcu_cols * geom.samp[c], geom.mcu_rows * geom.samp[c]
        dest = np.zeros((ph, pw, 64), np.int64)
        dest[:rh, :rw] = qv
        last_dc = 0
        for by in range(ph):                       # (only the DC needs the serial walk)
            for bx in range(pw):
                if by >= rh or bx >= rw:
                    dest[by, bx, 0] = last_dc      # dest_coeffs[0] = last_dc; the AC part stays zero
                last_dc = dest[by, bx, 0]
        padded.append(dest)
    # ---- EncodeScan's order: MCU rows, MCU columns, components, iy, ix
    my, mx = np.divmod(np.arange(geom.nmcu), geom.mcu_cols)
    cols = []
    for c in range(geom.ncomp):
        s = geom.samp[c]
        for iy in range(s):
            for ix in range(s):
                cols.append((c, iy, ix))
    G = geom.nmcu * geom.upm
    b_comp = np.tile(np.array([c for c, _, _ in cols]), geom.nmcu)
    b_iy = np.tile(np.array([iy for _, iy, _ in cols]), geom.nmcu)
    b_ix = np.tile(np.array([ix for _, _, ix in cols]), geom.nmcu)
    b_mcu = np.repeat(np.arange(geom.nmcu), geom.upm)
    b_my, b_mx = my[b_mcu], mx[b_mcu]
    samp = np.array(geom.samp)[b_comp]
    b_by, b_bx = b_my * samp + b_iy, b_mx * samp + b_ix
    zz = np.zeros((G, 64), np.int64)               # zig-zag order
    for c in range(geom.ncomp):
        m = b_comp == c
        zz[m] = padded[c][b_by[m], b_bx[m]][:, NATURAL]
    rw = np.array([g[0] for g in geom.grid])[b_comp]
    rh = np.array([g[1] for g in geom.grid])[b_comp]
    right, below = b_bx >= rw, b_by >= rh
    census["pad_block/right"] = int((right & ~below).sum())
    census["pad_block/below"] = int((below & ~right).sum())
    census["pad_block/corner"] = int((below & right).sum())
    first = (b_mcu == 0) & (b_ix == 0) & (b_iy == 0)
    census["dc_pred/none"] = int(first.sum())
    census["dc_pred/ix"] = int((b_ix > 0).sum())
    census["dc_pred/iy"] = int(((b_ix == 0) & (b_iy > 0)).sum())
    census["dc_pred/mx"] = int(((b_ix == 0) & (b_iy == 0) & (b_mx > 0)).sum())
    census["dc_pred/my"] = int(((b_ix == 0) & (b_iy == 0) & (b_mx == 0) & (b_my > 0)).sum())
    # ---- DC: the difference to the component's previous block in this order
    diff = np.zeros(G, np.int64)
    for c in range(geom.ncomp):
        idx = np.flatnonzero(b_comp == c)
        dc = zz[idx, 0]
        diff[idx] = dc - np.concatenate([[0], dc[:-1]])
    assert np.abs(diff).max() <= 32767 and np.abs(zz).max() <= 32767, "outside the domain (module docstring)"
    dc_n = _size(np.abs(diff))
    dc_extra = np.where(diff < 0, diff - 1, diff) & ((1 << dc_n) - 1)
    for n in range(13):
        for sign, m in (("pos", diff > 0), ("neg", diff < 0)) if n else (("zero", diff == 0),):
            census[f"dc_size/{n}/{sign}"] = int(((dc_n == n) & m).sum())
    census["dc_size/13to15/pos"] = int(((dc_n > 12) & (diff > 0)).sum())
    census["dc_size/13to15/neg"] = int(((dc_n > 12) & (diff < 0)).sum())
    # ---- AC: runs of zeros, ZRL, (run, size) symbols, end of block
    g_i, k_i = np.nonzero(zz[:, 1:])
    k_i = k_i + 1
    v = zz[g_i, k_i]
    same = np.concatenate([[False], g_i[1:] == g_i[:-1]])
    prev = np.where(same, np.concatenate([[0], k_i[:-1]]), 0)
    run = k_i - prev - 1
    zrl = run >> 4
    ac_n = _size(np.abs(v))
    ac_sym = ((run & 15) << 4) + ac_n
    ac_extra = np.where(v < 0, v - 1, v) & ((1 << ac_n) - 1)       # temp2 = ~temp for negative values
    last = np.zeros(G, np.int64)
    np.maximum.at(last, g_i, k_i)
    eob = last < 63
    cls = np.where(b_comp[g_i] == 0, 0, 1)
    for ci, name in enumerate(("luma", "chroma")):
        cnt = np.bincount(ac_sym[cls == ci], minlength=256)
        for r in range(16):
            for n in range(1, 12):
                census[f"ac_sym/{name}/{r:x}{n:x}"] = int(cnt[(r << 4) + n])
    census["ac_size/12to14"] = int((ac_n > 11).sum())
    for z in (1, 2, 3):
        census[f"zrl_per_coeff/{z}"] = int((zrl == z).sum())
    for r in (15, 16, 31, 32, 47, 48, 62):
        census[f"run_exact/{r}"] = int((run == r).sum())
    census["eob/alone"] = int((last == 0).sum())
    census["eob/after_62"] = int((last == 62).sum())
    census["eob/absent"] = int((last == 63).sum())
    census["eob/other"] = int(((last > 0) & (last < 62)).sum())
    a = np.abs(v)
    pow2 = (a & (a - 1)) == 0
    pow2m1 = (a & (a + 1)) == 0
    census["value/pos_pow2m1"] = int(((v >= 3) & pow2m1).sum())
    census["value/neg_pow2m1"] = int(((v <= -3) & pow2m1).sum())
    census["value/pos_pow2"] = int(((v >= 2) & pow2).sum())
    census["value/neg_pow2"] = int(((v <= -2) & pow2).sum())
    census["value/minus_one"] = int((v == -1).sum())
    # ---- the units in stream order: key = (block, zig-zag position, ZRLs before the symbol)
    zr_g, zr_k = np.repeat(g_i, zrl), np.repeat(k_i, zrl)
    zr_sub = np.arange(zrl.sum()) - np.repeat(np.cumsum(zrl) - zrl, zrl)
    e_g = np.flatnonzero(eob)
    parts = [  # (block, key within the block, table, symbol, extra bits, their number)
        (np.arange(G), np.zeros(G, np.int64), b_comp, dc_n, dc_extra, dc_n),
        (zr_g, zr_k * 8 + zr_sub, 3 + b_comp[zr_g], np.full(zr_g.size, 0xf0), np.zeros(zr_g.size, np.int64),
         np.zeros(zr_g.size, np.int64)),
        (g_i, k_i * 8 + 7, 3 + b_comp[g_i], ac_sym, ac_extra, ac_n),
        (e_g, np.full(e_g.size, 64 * 8), 3 + b_comp[e_g], np.zeros(e_g.size, np.int64), np.zeros(e_g.size, np.int64),
         np.zeros(e_g.size, np.int64)),
    ]
    key = np.concatenate([p[0] * 1024 + p[1] for p in parts])
    order = np.argsort(key, kind="stable")
    s = Symbols()
    s.geom = geom
    s.block = np.concatenate([p[0] for p in parts])[order]
    s.mcu = b_mcu[s.block]
    s.table, s.sym, s.extra, s.nbits = (np.concatenate([p[i] for p in parts])[order].astype(np.int64) for i in (2, 3, 4, 5))
    hist = np.zeros((2, 3, 256), np.int64)
    np.add.at(hist.reshape(6, 256), (s.table, s.sym), 1)
    s.hist = hist.astype(np.uint32)
    s.census = census
    return s


class Coded:
    pass


def encode(s, depth, code):
    """The units of `s` under (depth, code) [2][3][256] through the BitWriter."""
    geom = s.geom
    depth = np.asarray(depth, np.int64).reshape(6, 256)
    code = np.asarray(code, np.int64).reshape(6, 256)
    d = depth[s.table, s.sym]
    assert ((d >= 1) & (d <= 16)).all(), "a symbol in use without a code of 1..16 bits"
    cd = code[s.table, s.sym]
    assert (cd >> d == 0).all()
    ln = d + s.nbits
    val = (cd << s.nbits) | s.extra
    end = np.cumsum(ln)
    pos = end - ln
    total = int(end[-1])
    pad = (-total) % 8                              # JumpToByteBoundary: ones up to the byte boundary
    bits = np.zeros(total + pad, np.uint8)
    for k in range(int(ln.max())):
        m = ln > k
        bits[pos[m] + k] = (val[m] >> (ln[m] - 1 - k)) & 1
    bits[total:] = 1
    raw = np.packbits(bits)
    is_ff = raw == 0xff
    r = Coded()
    r.hist = s.hist
    r.bits_per_mcu = np.bincount(s.mcu, weights=ln, minlength=geom.nmcu).astype(np.int64)
    r.total_bits = total
    r.unstuffed = raw.tobytes()
    r.stuffed_count = int(is_ff.sum())
    r.stuffed = np.insert(raw, np.flatnonzero(is_ff) + 1, 0).tobytes()   # EmitByte: 0x00 after every 0xFF
    # ---- census of the placement
    c = dict(s.census)
    L = geom.layout
    m_end = np.cumsum(r.bits_per_mcu)
    m_start = m_end - r.bits_per_mcu
    phase = m_start % 32
    span = phase + r.bits_per_mcu
    span[-1] += pad                                 # the last MCU also writes the padding
    words = (span + 31) // 32
    cnt = np.bincount(phase, minlength=32)
    for p in range(32):
        c[f"mcu_phase/{p}"] = int(cnt[p])
    c["mcu_words/1"], c["mcu_words/2"], c["mcu_words/3plus"] = (int((words == 1).sum()), int((words == 2).sum()),
                                                                  int((words >= 3).sum()))
    inner = np.ones(geom.nmcu, bool)
    inner[-1] = False
    c["mcu_in_one_word_shared_with_both_neighbours"] = int(((words == 1) & (phase != 0) & (m_end % 32 != 0) & inner).sum())
    c["unit_straddles_word"] = int(((pos >> 5) != ((end - 1) >> 5)).sum())
    c["unit_ends_on_word"] = int((end % 32 == 0).sum())
    for lay in ("444", "420", "gray"):
        c[f"mcu_span/{lay}/le8192"] = int((span <= STAGE_BITS).sum()) if lay == L else 0
        c[f"mcu_span/{lay}/gt8192"] = int((span > STAGE_BITS).sum()) if lay == L else 0
    c["mcu_span/420/within64_below"] = int(((span > STAGE_BITS - 64) & (span <= STAGE_BITS)).sum()) if L == "420" else 0
    c["mcu_span/420/within64_above"] = int(((span > STAGE_BITS) & (span <= STAGE_BITS + 64)).sum()) if L == "420" else 0
    for k in range(8):
        c[f"final_pad/{k}"] = int(pad == k)
    ff_at = np.flatnonzero(is_ff)
    for j in range(4):
        c[f"ff_at_byte/{j}"] = int((ff_at % 4 == j).sum())
    c["ff_last_byte"] = int(is_ff[-1])
    mark = np.zeros(total + pad + 1, np.int64)      # bits that belong to a code (not extra bits, not padding)
    np.add.at(mark, pos, 1)
    np.add.at(mark, pos + d, -1)
    code_bytes = np.packbits(np.cumsum(mark)[:-1] > 0)
    c["ff_from_code_bits"] = int((is_ff & (code_bytes == 0xff)).sum())
    for k in range(4):
        c[f"nbytes_mod4/{k}"] = int(raw.size % 4 == k)
    tiles = -(-geom.nmcu // SCAN_TILE)
    c["tiles/1"], c["tiles/2"], c["tiles/3to64"] = int(tiles == 1), int(tiles == 2), int(3 <= tiles <= 64)
    c["tiles/gt64"], c["tiles/gt128"] = int(tiles > 64), int(tiles > 128)
    lw = (geom.nmcu - 1) % MCU_PER_WAVE + 1
    lg = (-(-geom.nmcu // MCU_PER_WAVE) - 1) % MCU_WAVES + 1
    for k in range(1, 5):
        c[f"last_wave_mcus/{k}"] = int(lw == k)
        c[f"last_group_waves/{k}"] = int(lg == k)
    c["nmcu_gt4096"] = int(geom.nmcu > 4096)
    r.census = c
    r.span = span
    r.pad = pad
    r.ff_at = ff_at
    return r


# ------------------------------------------------------------------------------ code tables ----
KINDS = ("optimal", "flat16", "skewed")


def check_prefix_code(depth, code, used):
    """Every symbol of `used` (bool [256]) has a code of 1..16 bits, and no code is a prefix of another."""
    syms = np.flatnonzero(used)
    words = []
    for sy in syms:
        d, cd = int(depth[sy]), int(code[sy])
        assert 1 <= d <= 16 and cd >> d == 0, (sy, d, cd)
        words.append(format(cd, "0%db" % d))
    words.sort()
    for a, b in zip(words, words[1:]):
        assert not b.startswith(a), (a, b)


def _flat16(used):
    depth, code = np.zeros(256, np.uint8), np.zeros(256, np.uint16)
    syms = np.flatnonzero(used)
    depth[syms] = 16
    code[syms] = (0x9e37 * (np.arange(syms.size) + 1)) & 0xffff     # an odd multiplier: distinct 16-bit values
    return depth, code


def _skewed(hist, is_ac):
    """Depths 1..16 as far as Kraft's inequality lets the table have them, every other symbol at 16; ZRL, EOB and the
    most frequent symbol at depth 16 with the codes 0xFFFF, 0xFFFE, 0xFFFD.  The short codes are canonical (first
    come, first served from 0 upwards), the 16-bit ones are taken from the top of the code space downwards, inside the
    part the short codes leave free."""
    used = hist > 0
    special = []
    if is_ac:
        used = used.copy()
        used[0xf0] = used[0] = True       # the kernels load these two codes whether the frame has the symbols or not
        special = [0xf0, 0]
    h = hist.astype(np.int64).copy()
    h[special] = -1
    if (h > 0).any():
        special.append(int(np.argmax(h)))
    rest = sorted((sy for sy in np.flatnonzero(used) if sy not in special), key=lambda sy: (sy * 73 + 11) % 257)
    depth, code = np.zeros(256, np.uint8), np.zeros(256, np.uint16)
    free = 1 << 16                        # in units of 2^-16
    nxt = 1                               # next depth of the ladder
    short = []
    for i, sy in enumerate(rest):
        need_after = len(rest) - i - 1 + len(special)
        d = nxt
        while d < 16 and free - (1 << (16 - d)) < need_after:
            d += 1
        depth[sy] = d
        free -= 1 << (16 - d)
        if d < 16:
            short.append(sy)
            nxt = d + 1
    assert free >= len(special)
    c = 0                                 # canonical codes for the short ones, in order of depth
    prev_d = 0
    for sy in sorted(short, key=lambda sy: depth[sy]):
        c <<= int(depth[sy]) - prev_d
        code[sy] = c
        c += 1
        prev_d = int(depth[sy])
    top = 0xffff
    for sy in special + [sy for sy in rest if depth[sy] == 16]:
        depth[sy] = 16
        code[sy] = top
        top -= 1
    return depth, code, used


def tables(kind, hist, optimal=None):
    """(depth, code) uint8 / uint16 [2][3][256] of `kind` for a frame with the symbol counts `hist`.  optimal: the pair
    the product builds (jpeg_head), for kind 'optimal'."""
    if kind == "optimal":
        return optimal
    depth, code = np.zeros((2, 3, 256), np.uint8), np.zeros((2, 3, 256), np.uint16)
    for t in range(2):
        for c in range(3):
            if kind == "flat16":
                used = hist[t, c] > 0
                if t == 1:
                    used = used.copy()
                    used[0xf0] = used[0] = True
                depth[t, c], code[t, c] = _flat16(used)
            else:
                depth[t, c], code[t, c], used = _skewed(hist[t, c], t == 1)
            check_prefix_code(depth[t, c], code[t, c], used)
    return depth, code


# --------------------------------------------------------------------------------- families ----
def _magnitudes(rng, sizes):
    """A random value of each given size (bits of the magnitude), random sign."""
    sizes = np.asarray(sizes, np.int64)
    lo = np.where(sizes > 0, 1 << np.maximum(sizes - 1, 0), 0)
    mag = lo + (rng.random(sizes.shape) * lo).astype(np.int64)
    mag = np.minimum(mag, (1 << sizes) - 1)
    return np.where(rng.random(sizes.shape) < 0.5, -mag, mag)


def _scan_order(geom, c):
    """Raster indices of component c's REAL blocks in the order the scan visits them."""
    rw, rh = geom.grid[c]
    s = geom.samp[c]
    out = []
    for my in range(geom.mcu_rows):
        for mx in range(geom.mcu_cols):
            for iy in range(s):
                for ix in range(s):
                    by, bx = my * s + iy, mx * s + ix
                    if by < rh and bx < rw:
                        out.append(by * rw + bx)
    return np.array(out)


def _mcu_of_blocks(geom, c):
    rw, rh = geom.grid[c]
    s = geom.samp[c]
    by, bx = np.divmod(np.arange(rw * rh), rw)
    return (by // s) * geom.mcu_cols + bx // s


def _zeros(geom):
    return [np.zeros((gw * gh, 64), np.int64) for gw, gh in geom.grid]


def _sparse_ac(geom, rng, density, max_size):
    zq = _zeros(geom)
    for z in zq:
        v = _magnitudes(rng, rng.integers(1, max_size + 1, z.shape))
        v[rng.random(z.shape) >= density] = 0
        z[:] = v
        z[:, 0] = rng.integers(-255, 256, z.shape[0])
    return zq


AC_SYMBOLS = [(r, n) for n in range(1, 12) for r in range(16)]


def fam_symbols_cyclic(geom, rng):
    """Blocks filled with the (run, size) symbols in a fixed cyclic order, each block starting elsewhere in it."""
    zq = _sparse_ac(geom, rng, 0.0, 1)
    for c, z in enumerate(zq):
        for b in range(z.shape[0]):
            i = (b * 7 + 29 * c) % len(AC_SYMBOLS)
            k = 0
            while True:
                r, n = AC_SYMBOLS[i]
                if k + r + 1 > 63:
                    break
                k += r + 1
                z[b, k] = _magnitudes(rng, np.array([n]))[0]
                i = (i + 1) % len(AC_SYMBOLS)
    return zq, None


def fam_symbols_single(geom, rng):
    """One AC symbol per block, behind 0..3 ZRLs, the end-of-block code right after it."""
    zq = _sparse_ac(geom, rng, 0.0, 1)
    for c, z in enumerate(zq):
        for b in range(z.shape[0]):
            r, n = AC_SYMBOLS[(b + 59 * c) % len(AC_SYMBOLS)]
            k = r + 1 + 16 * ((b // len(AC_SYMBOLS) + b) % 4)
            if k > 63:
                k = r + 1
            z[b, k] = _magnitudes(rng, np.array([n]))[0]
    return zq, None


RUNS = (15, 16, 31, 32, 47, 48, 62)


def fam_runs_exact(geom, rng):
    """Runs of exactly 15, 16, 31, 32, 47, 48 and 62 zeros, from the block's start and behind a coefficient; blocks whose
    last coefficient sits at 62, at 63, and blocks without any."""
    zq = _sparse_ac(geom, rng, 0.0, 1)
    for c, z in enumerate(zq):
        for b in range(z.shape[0]):
            j = (b + 3 * c) % 17
            val = lambda: _magnitudes(rng, rng.integers(1, 9, 1))[0]   # noqa: E731
            if j < 7:
                z[b, RUNS[j] + 1] = val()
            elif j < 13:
                z[b, 1] = val()
                z[b, RUNS[j - 7] + 2] = val()
            elif j == 13:
                z[b, 62] = val()
            elif j == 14:
                z[b, 63] = val()
            elif j == 15:
                z[b, 5], z[b, 62], z[b, 63] = val(), val(), val()
    return zq, None


def fam_runs_random(geom, rng):
    return _sparse_ac(geom, rng, 0.07, 9), None


DC_LADDER = sorted({(1 << k) - 1 for k in range(12)} | {1 << k for k in range(12)})


def fam_dc_ladder(geom, rng):
    """DC differences of +-(2^k - 1) and +-2^k for k = 0..11 along every component's scan order: the DCs are m, 0, m', 0,
    ... with m from that ladder (a padding block in between repeats the DC before it and changes no difference)."""
    zq = _sparse_ac(geom, rng, 0.05, 6)
    for c, z in enumerate(zq):
        order = _scan_order(geom, c)
        i = np.arange(order.size)
        z[order, 0] = np.where(i % 2 == 0, np.array(DC_LADDER)[(i // 2 + 5 * c) % len(DC_LADDER)], 0)
    return zq, None


def fam_dc_extremes(geom, rng):
    """+2047 and -2047 alternating along the scan order."""
    zq = _sparse_ac(geom, rng, 0.05, 6)
    for c, z in enumerate(zq):
        order = _scan_order(geom, c)
        z[order, 0] = np.where((np.arange(order.size) + c) % 2 == 0, 2047, -2047)
    return zq, None


def fam_wide(geom, rng):
    """Magnitudes up to 16383 (AC sizes up to 14) and DCs within +-16383 (difference sizes up to 15): a code of 16
    bits and its extra bits make 31 bits."""
    zq = _sparse_ac(geom, rng, 0.3, 14)
    for c, z in enumerate(zq):
        order = _scan_order(geom, c)
        dc = rng.integers(-16383, 16384, order.size)
        dc[::3] = np.where(np.arange(dc[::3].size) % 2 == 0, 16383, -16383)
        z[order, 0] = dc
        z[::5, 63] = 16383
        z[1::5, 1] = -16383
    return zq, None


def fam_sparse(geom, rng):
    """Almost every block is a DC difference of zero and an end-of-block code."""
    zq = _sparse_ac(geom, rng, 0.0, 1)
    for z in zq:
        z[:, 0] = 3
        hit = rng.random(z.shape[0]) < 0.04
        z[hit, 1 + rng.integers(0, 63, int(hit.sum()))] = 1
        z[::97, 0] = 4
    return zq, None


def fam_dense(geom, rng):
    """No zero anywhere.  The sizes of an MCU's coefficients add up to 1900 + (37 * mcu) % 300 in a 4:2:0 frame (the same
    share per block elsewhere): under 16-bit codes the 4:2:0 MCUs are 6 * 64 * 16 bits + that sum + their DC sizes long
    and sweep across the staging limit of 8192 bits one bit at a time."""
    zq = _zeros(geom)
    per_mcu = 1900 + (37 * np.arange(geom.nmcu)) % 300
    for c, z in enumerate(zq):
        mcu = _mcu_of_blocks(geom, c)
        s2 = geom.samp[c] ** 2
        # this block's share of the MCU's sum: six shares, the first (sum % 6) of them one larger
        rw = geom.grid[c][0]
        by, bx = np.divmod(np.arange(z.shape[0]), rw)
        slot = (0 if c == 0 else 2 + c) if geom.layout == "420" else 2 * c
        slot = slot + (by % geom.samp[c]) * geom.samp[c] + bx % geom.samp[c] if s2 > 1 else np.full(z.shape[0], slot)
        share = per_mcu[mcu] // 6 + (slot < per_mcu[mcu] % 6)
        sizes = (share // 63)[:, None] + (np.arange(63)[None, :] < (share % 63)[:, None])
        z[:, 1:] = _magnitudes(rng, sizes)
        z[:, 0] = rng.integers(-3, 4, z.shape[0])
    return zq, None


def fam_phase_tiny(geom, rng):
    """Every block a zero DC difference and an end-of-block: the shortest MCUs there are, many to a word."""
    zq = _zeros(geom)
    for z in zq:
        z[:, 0] = -7
    return zq, None


def fam_phase_walk(geom, rng):
    """MCU lengths that differ by the DC difference's size from one to the next: start phases drift through a word."""
    zq = _zeros(geom)
    for c, z in enumerate(zq):
        order = _scan_order(geom, c)
        i = np.arange(order.size)
        z[order, 0] = np.where(i % 2 == 0, 0, 1 << ((i // 2 + c) % 11))
        z[::3, 1 + (np.arange(z[::3].shape[0]) % 5)] = 1
    return zq, None


def fam_ff_ones(geom, rng):
    """Positive values 2^n - 1, n = 8..11: their extra bits are all ones.  The last coefficient of the scan is 2047, so
    that the stream ends in ones and the padding completes a last byte of 0xFF."""
    zq = _zeros(geom)
    for z in zq:
        z[:, 1:] = (1 << rng.integers(8, 12, (z.shape[0], 63))) - 1
        z[:, 1:][rng.random((z.shape[0], 63)) < 0.3] = 0
        z[:, 0] = rng.integers(-3, 4, z.shape[0])
        z[:, 63] = 2047
    return zq, None


def fam_ff_code(geom, rng):
    """Negative values -(2^n - 1): their extra bits are all zeros, a 0xFF byte can only come from code bits."""
    zq = _zeros(geom)
    for z in zq:
        v = -((1 << rng.integers(1, 7, (z.shape[0], 63))) - 1)
        v[rng.random(v.shape) < 0.5] = 0
        z[:, 1:] = v
        z[:, 0] = 0
    return zq, None


def _raw(geom, rng, lo, hi, density):
    """Dequantised coefficients drawn directly (not multiples of q)."""
    out = []
    for gw, gh in geom.grid:
        v = rng.integers(lo, hi + 1, (gw * gh, 64))
        v[:, 1:][rng.random((gw * gh, 63)) >= density] = 0
        out.append(v)
    return out


def fam_quant_one(geom, rng):
    return _raw(geom, rng, -2047, 2047, 0.4), np.ones((3, 64), np.int64)


def fam_quant_huge(geom, rng):
    """q larger than every coefficient: everything quantises to zero."""
    return _raw(geom, rng, -2047, 2047, 0.6), np.full((3, 64), 2048, np.int64)


def fam_quant_remainders(geom, rng):
    """Coefficients that are no multiples of q, of both signs: C++ `/` truncates towards zero."""
    q = np.stack([rng.integers(2, 9, 64), rng.integers(2, 30, 64), rng.integers(2, 30, 64)])
    raw = _raw(geom, rng, -2047, 2047, 0.5)
    for c, v in enumerate(raw):           # ... with -(q - 1), -q, -(q + 1) and their positives among them
        qn = q[c][None, :]
        pick = rng.integers(0, 12, v.shape)
        for j, val in enumerate((-(qn - 1), -qn, -(qn + 1), qn - 1, qn, qn + 1)):
            v[:] = np.where(pick == j, np.broadcast_to(val, v.shape), v)
    return raw, q


def fam_quant_255(geom, rng):
    raw = _raw(geom, rng, -32768, 32767, 0.5)
    for v in raw:
        v[::7, 2] = -32768
        v[1::7, 2] = 32767
    return raw, np.full((3, 64), 255, np.int64)


def fam_quant_4000(geom, rng):
    raw = _raw(geom, rng, -32768, 32767, 0.5)
    for v in raw:
        v[::7, 2] = -32768
        v[1::7, 0] = -32768
    return raw, np.full((3, 64), 4000, np.int64)


def _fam_pad(k):
    def fam(geom, rng):
        """Sparse content whose final padding is k bits under 16-bit codes: there the scan's length is 16 bits per
        symbol plus the sizes, and one coefficient's size settles the sum modulo 8."""
        zq = _sparse_ac(geom, rng, 0.1, 7)
        zq[0][0, 1] = 1
        blocks, q = _finish(geom, zq, None)
        s = symbolize(geom, blocks, q)
        total = 16 * s.sym.size + int(s.nbits.sum())
        want = (-k) % 8                  # total bits modulo 8 that leaves k bits of padding
        n = 1 + (want - total) % 8       # the new size of that coefficient (it had size 1)
        zq[0][0, 1] = (1 << n) - 1
        return zq, None
    return fam


def _finish(geom, zq, q):
    """Quantised values in zig-zag order (q None: times a q that varies by position) or raw coefficients -> dequantised
    int16 blocks in natural order, q [3][64]."""
    if q is None:
        big = max(int(np.abs(z).max()) for z in zq)
        q = np.ones((3, 64), np.int64)
        if big <= 2047:                    # 2047 * 16 stays inside int16
            q = np.stack([1 + (np.arange(64) * (c + 3)) % 16 for c in range(3)])
            if big > 1023:
                q = np.minimum(q, 15)
        elif big <= 16383:
            q = np.stack([1 + (np.arange(64) + c) % 2 for c in range(3)])
        blocks = []
        for c, z in enumerate(zq):
            nat = np.zeros(z.shape, np.int64)
            nat[:, NATURAL] = z
            blocks.append(nat * q[c][None, :])
    else:
        blocks = zq
    out = []
    for b in blocks:
        assert b.min() >= -32768 and b.max() <= 32767
        out.append(b.astype(np.int16))
    return out, np.asarray(q, np.int32)


FAMILIES = {
    "symbols/cyclic": fam_symbols_cyclic,
    "symbols/single": fam_symbols_single,
    "runs/exact": fam_runs_exact,
    "runs/random": fam_runs_random,
    "dc/ladder": fam_dc_ladder,
    "dc/extremes": fam_dc_extremes,
    "wide": fam_wide,
    "sparse": fam_sparse,
    "dense": fam_dense,
    "phase/tiny": fam_phase_tiny,
    "phase/walk": fam_phase_walk,
    "ff/ones": fam_ff_ones,
    "ff/code": fam_ff_code,
    "quant/one": fam_quant_one,
    "quant/huge": fam_quant_huge,
    "quant/remainders": fam_quant_remainders,
    "quant/255": fam_quant_255,
    "quant/4000": fam_quant_4000,
}
FAMILIES.update({f"pad/{k}": _fam_pad(k) for k in range(8)})


class Case:
    pass


@functools.lru_cache(maxsize=24)
def case(name, layout, w, h, seed=0):
    """The family `name` on a (layout, w, h) frame: coefficients (blocks per component and as the frame's array), q, and
    the reference coder's symbols."""
    geom = Geom(layout, w, h)
    rng = np.random.default_rng(zlib.crc32(f"{name}/{layout}/{w}x{h}/{seed}".encode()))
    zq, q = FAMILIES[name](geom, rng)
    c = Case()
    c.name, c.geom = name, geom
    c.blocks, c.q = _finish(geom, zq, q)
    if geom.ncomp == 3 and not (c.blocks[1].any() or c.blocks[2].any()):
        c.blocks[1][0, 1] = c.q[1][1]     # a writer drops chroma components that are entirely zero
    c.coeffs = geom.coeff_array(c.blocks)
    c.multiples_of_q = all((b.astype(np.int64) % c.q[i][None, :] == 0).all() for i, b in enumerate(c.blocks))
    c.symbols = symbolize(geom, c.blocks, c.q)
    return c
