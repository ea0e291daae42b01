"""Synthetic inputs of the frame path -- the code that turns pixels into coefficients and coefficients back into
pixels: k_encode_rgb, k_quantize, k_reconstruct, k_reconstruct_listed, k_chroma_samples + k_reconstruct420,
k_to_float_pixels, k_set_downsampled_coeffs and the k_pp_* kernels of gz_downsample.  Deterministic, file-free (but for
the photograph control), fixed seeds.  tests/test_frame_domain.py counts, with the oracle's frame_* census, which arm
of which value branch each family takes; tests/parity_cases.py (case_frame_*) runs them through a library.

  coefficient families  coeff_cases(w, h, layout)   -> (name, coefficients in the frame layout)
  quantiser tables      quant_tables(coeffs, layout, w, h) -> (name, int32 [3][64])
  pixel families        pixel_cases(w, h) / lattice_image()
  float planes          plane_cases(w, h) / tie_planes()
  YUV fields            yuv_cases(w, h)             -> (name, 4:4:4 coefficients whose ToFloatPixels planes are the field)

Magnitudes.  The reference's integer IDCT (idct.cc:41-137) accumulates products of a matrix row with eight int16
values in an `int`, one term after the other: every partial sum is bounded by sum_u |M[x][u]| * max|in| <=
61213 * 32768 = 2 005 827 584, and with the rounding constants (2^10, 257 << 17 = 33 685 504) stays below 2^31 =
2 147 483 648 in both passes, whatever the int16 inputs are.  idct_sums_fit_int32() evaluates that bound on the
actual coefficients, in int64, with the int16 wrap applied between the passes; the tests assert it on every family."""
import typing

import numpy as np

import images
from checkers import oracle

SEED = 20261019

# Contexts need w, h >= 8.  (64, 8) / (72, 8): one full strip of eight blocks, one strip and one block.
CTX_SIZES = [(8, 8), (9, 8), (8, 9), (15, 16), (16, 15), (17, 17), (12, 10), (24, 9), (65, 9), (93, 59),
             (64, 8), (72, 8)]
# ... the context-free entries (encode_rgb_only, component_to_float_pixels, component_set_downsampled, decode_coeffs) also:
FREE_SIZES = [(1, 1), (1, 9), (9, 1), (2, 3), (7, 7)]
MID_SIZE = (93, 59)

# idct.cc:29-38
IDCT_M = np.array([
    [8192, 11363, 10703, 9633, 8192, 6437, 4433, 2260],
    [8192, 9633, 4433, -2259, -8192, -11362, -10704, -6436],
    [8192, 6437, -4433, -11362, -8192, 2261, 10704, 9633],
    [8192, 2260, -10703, -6436, 8192, 9633, -4433, -11363],
    [8192, -2260, -10703, 6436, 8192, -9633, -4433, 11363],
    [8192, -6437, -4433, 11362, -8192, -2261, 10704, -9633],
    [8192, -9633, 4433, 2259, -8192, 11362, -10704, 6436],
    [8192, -11363, 10703, -9633, 8192, -6437, 4433, -2260]], np.int64)


def grid(w, h):
    bw, bh = (w + 7) // 8, (h + 7) // 8
    cbw, cbh = (w + 15) // 16, (h + 15) // 16
    return bw, bh, bw * bh, cbw, cbh, cbw * cbh


def comp_sizes(w, h, layout):
    _, _, nb, _, _, nbc = grid(w, h)
    return [nb, nb, nb] if layout == "444" else [nb, nbc, nbc]


def idct_blocks_int64(blocks):
    """ComputeBlockIDCT (idct.cc:139-161) of [n][64] int16 blocks in int64 numpy -> (pixels u8 [n][64], the largest
    sum of magnitudes any partial sum of either pass is bounded by, how many column results left int16)."""
    b = np.asarray(blocks, np.int16).reshape(-1, 8, 8).astype(np.int64)          # [n][u][x]
    absm = np.abs(IDCT_M)
    col = np.einsum("yu,nux->nyx", IDCT_M, b)
    bound = np.einsum("yu,nux->nyx", absm, np.abs(b)).max(initial=0) + (1 << 10)
    col = (col + (1 << 10)) >> 11
    wrapped = int(((col < -32768) | (col > 32767)).sum())
    col = ((col + 32768) & 0xffff) - 32768                                      # the (int16) store
    row = np.einsum("xu,nyu->nyx", IDCT_M, col)
    bound = max(bound, np.einsum("xu,nyu->nyx", absm, np.abs(col)).max(initial=0) + (257 << 17))
    px = np.clip((row + (257 << 17)) >> 18, 0, 255).astype(np.uint8)
    return px.reshape(-1, 64), int(bound), wrapped


def idct_sums_fit_int32(coeffs):
    """The assertion on the inputs: no sum of the reference's IDCT of these blocks can leave int32."""
    _, bound, _ = idct_blocks_int64(np.asarray(coeffs, np.int16).reshape(-1, 64))
    return bound < (1 << 31)


# ---------------------------------------------------------------- coefficient families --
MAGS = (1024, 4096, 16384, 32767)


def _sparse(p):
    """frame_idct_*: one large coefficient at position p % 64, the sign by p // 64 % 2, four magnitudes (-32768 among
    them): 512 patterns.  A single coefficient reaches the clamps of the row pass alone, and from 16384 on its
    column result leaves int16 (8192 * 16384 >> 11 = 65536)."""
    b = np.zeros(64, np.int64)
    k, neg, m = p % 64, (p // 64) % 2, MAGS[(p // 128) % 4]
    b[k] = -m - (m == 32767) if neg else m
    return b


def _matrix_rows(p):
    """frame_idct_column_wraps_int16, both pixel clamps: sign patterns copied from rows r1 (down the columns) and r2
    (along the rows) of the IDCT matrix, so that the sums of output (r2, r1) add without cancellation; magnitudes 256,
    2048, 16384, 32767: 256 patterns."""
    r1, r2, m = p % 8, (p // 8) % 8, (256, 2048, 16384, 32767)[(p // 64) % 4]
    return (np.sign(IDCT_M[r1])[:, None] * np.sign(IDCT_M[r2])[None, :]).reshape(64) * m


def _dc_ramp(p):
    """frame_idct_pixel_clamped_low / _high / _inside: DC only, pixel = 128 + DC / 8 from -52 to 308 in 97 steps."""
    b = np.zeros(64, np.int64)
    b[0] = -1440 + 30 * (p % 97)
    return b


def _wrap(p, rng):
    """frame_idct_column_wraps_int16 beside _fits: dense blocks over the whole int16 range (column sums of hundreds of
    millions, >> 11 far outside int16), every third with its first row at the extremes."""
    b = rng.integers(-32768, 32768, 64)
    if p % 3 == 0:
        b[:8] = np.where(np.arange(8) & 1, -32768, 32767)
    return b


def _family_blocks(name, n, c, rng, shift):
    gen = {"sparse": _sparse, "matrix_rows": _matrix_rows, "dc_ramp": _dc_ramp}
    out = np.zeros((n, 64), np.int64)
    for i in range(n):
        p = i + 43 * c + shift
        out[i] = _wrap(p, rng) if name == "wrap" else gen[name](p)
    return out


def _extreme_chroma(n, c, rng, reverse):
    """frame_rgb444_* / frame_rgb420_*: chroma DC at the extremes (pixels 0 and 255 and beyond) with mid luma -- every
    R/G/B clamp of ycc_to_rgb, low and high -- and the reverse, luma at the extremes with mid chroma; a little AC on
    top so that the blocks are not flat."""
    out = np.zeros((n, 64), np.int64)
    i = np.arange(n)
    ext = np.array([-1100, 1100, -1024, 1016, -600, 600, 0, 300])
    if (c == 0) == reverse:
        out[:, 0] = ext[(i + 3 * c) % 8] if c else ext[i % 8]
        if c == 2:
            out[:, 0] = ext[(i // 8 + i) % 8]   # Cb and Cr walk their extremes independently
    else:
        out[:, 0] = (i % 5 - 2) * 40
    out[:, 1:6] = rng.integers(-60, 61, (n, 5))
    return out


COEFF_FAMILIES = ("sparse", "matrix_rows", "dc_ramp", "chroma_extreme", "luma_extreme", "wrap", "photo")


def photo_coeffs(w, h, layout):
    """The control: a photograph's coefficients, quantised by 3 (what every other test of the frame path runs on)."""
    rgb = images.crop(w, h, 120, 60)
    co = oracle.encode_rgb(rgb)
    q = np.full((3, 64), 3, np.int32)
    if layout == "444":
        return oracle.reconstruct(co, w, h, q)[0]
    return oracle.reconstruct420(oracle.downsample(co, w, h), w, h, q)[0]


def coeffs_of(name, w, h, layout):
    """Family `name` in the frame layout: int16 [3][nb][64] (4:4:4) or [nb + 2 nbc][64] (4:2:0)."""
    if name == "photo":
        return photo_coeffs(w, h, layout)
    rng = np.random.default_rng(SEED + COEFF_FAMILIES.index(name) * 1000 + 31 * w + h)
    parts = []
    for c, n in enumerate(comp_sizes(w, h, layout)):
        if name in ("chroma_extreme", "luma_extreme"):
            parts.append(_extreme_chroma(n, c, rng, reverse=name == "luma_extreme"))
        else:
            parts.append(_family_blocks(name, n, c, rng, shift=7 * (w + h)))
    co = np.concatenate(parts).astype(np.int16)
    return co.reshape(3, -1, 64) if layout == "444" else co


def coeff_cases(w, h, layout, only=None):
    for name in COEFF_FAMILIES:
        if only is None or name in only:
            yield name, coeffs_of(name, w, h, layout)


def luma_extreme_blocks(n, shift=0):
    """Luma blocks for the comparison of the IDCT copies with each other: sparse, matrix_rows and wrap in turn."""
    rng = np.random.default_rng(SEED + 77 + n)
    out = np.zeros((n, 64), np.int64)
    for i in range(n):
        p = i + shift
        out[i] = (_sparse(5 * p), _matrix_rows(3 * p), _wrap(p, rng))[i % 3]
    return out.astype(np.int16)


# -------------------------------------------------------------------- quantiser tables --
PRIMES = np.array([2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101,
                   103, 107, 109, 113, 127, 131, 137, 139, 149, 151, 157, 163, 167, 173, 179, 181, 191, 193, 197, 199,
                   211, 223, 227, 229, 233, 239, 241, 251, 257, 263, 269, 271, 277, 281, 283, 293, 307, 311], np.int32)
QUANT_TABLES = ("ones", "primes", "ties", "large", "per_component")


def quant_table(name, coeffs, layout, w, h):
    """int32 [3][64].
    ones           q = 1: nothing moves (frame_quant_toward_zero with r = 0)
    primes         a prime per coefficient, rotated per component: round up / down / toward zero
    ties           q = 2|raw|, 2|raw| - 1, 2|raw| + 1 by position, raw = the coefficient of the component's first,
                   middle or last block: frame_quant_tie_positive / _negative and both neighbours of a tie
    large          255, 32767, 40000, 65535 by position, rotated per component: frame_quant_q_above_raw, and
                   frame_quant_wrapped_int16 (raw = 30000, q = 40000: 2r > q, raw + q - r = 40000 wraps)
    per_component  three flat tables 3, 7, 16: a component boundary b1 / b2 off by a block shows"""
    k = np.arange(64)
    if name == "ones":
        return np.ones((3, 64), np.int32)
    if name == "primes":
        return np.stack([np.roll(PRIMES, 5 * c) for c in range(3)]).astype(np.int32)
    if name == "large":
        big = np.array([255, 32767, 40000, 65535], np.int32)
        return np.stack([big[(k + c) % 4] for c in range(3)]).astype(np.int32)
    if name == "per_component":
        return np.stack([np.full(64, v) for v in (3, 7, 16)]).astype(np.int32)
    assert name == "ties"
    co = np.asarray(coeffs, np.int16).reshape(-1, 64).astype(np.int64)
    q = np.ones((3, 64), np.int64)
    first = 0
    for c, n in enumerate(comp_sizes(w, h, layout)):
        for kk in range(64):
            raw = co[first + (0, n // 2, n - 1)[kk % 3], kk]
            q[c, kk] = max(1, 2 * abs(raw) + ((kk // 3) % 3 - 1))
        first += n
    return q.astype(np.int32)


def quant_tables(coeffs, layout, w, h, only=None):
    for name in QUANT_TABLES:
        if only is None or name in only:
            yield name, quant_table(name, coeffs, layout, w, h)


def quantize_by_definition(coeffs, q, layout, w, h):
    """quantize.h:24-29 per block through the oracle's orc_quantize_block, component by component."""
    co = np.asarray(coeffs, np.int16).reshape(-1, 64)
    out = np.zeros_like(co)
    first = 0
    for c, n in enumerate(comp_sizes(w, h, layout)):
        for b in range(first, first + n):
            out[b] = oracle.quantize_block(co[b], q[c])[0]
        first += n
    return out.reshape(np.asarray(coeffs).shape)


# ---------------------------------------------------------------------- pixel families --
LATTICE = (0, 16, 32, 48, 64, 80, 96, 112, 128, 144, 160, 176, 192, 208, 224, 240, 255)


def lattice_image():
    """frame_encode_pixel_inside, k_encode_rgb's colour transform: one constant 8x8 block per colour, the 17^3 lattice
    and 2000 seeded colours (6913 blocks, 84 blocks wide): the DC of every block shows the converted value."""
    lat = np.array(np.meshgrid(LATTICE, LATTICE, LATTICE, indexing="ij"), np.uint8).reshape(3, -1).T
    rnd = np.random.default_rng(SEED + 1).integers(0, 256, (2000, 3)).astype(np.uint8)
    cols = np.concatenate([lat, rnd])
    bw = 84
    bh = -(-len(cols) // bw)
    pad = np.concatenate([cols, np.zeros((bw * bh - len(cols), 3), np.uint8)]).reshape(bh, bw, 3)
    return np.ascontiguousarray(np.repeat(np.repeat(pad, 8, axis=0), 8, axis=1))


PRIMARIES = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255],
                      [0, 0, 0], [255, 255, 255]], np.uint8)
# (w % 8, h % 8 in {1, 7}: one replicated column / row, and seven)
PIXEL_SIZES = [(9, 9), (15, 15), (9, 15), (15, 9), (17, 23), (23, 17), (25, 31), (31, 25)]


def pixel_cases(w, h):
    """frame_encode_x_replicated / _y_replicated: saturated-primary checkerboards at period 1 and 2 (the last column and
    row, which the edge replication repeats, differ from their neighbours) and seeded noise."""
    y, x = np.mgrid[0:h, 0:w]
    for period in (1, 2):
        yield f"primaries/period{period}", np.ascontiguousarray(PRIMARIES[((x // period) + 3 * (y // period)) % 8])
    yield "noise", np.random.default_rng(SEED + 2 + 31 * w + h).integers(0, 256, (h, w, 3)).astype(np.uint8)


# ------------------------------------------------------------------------ float planes --
# What SetDownsampledCoefficients is given after PreProcessChannel: a channel of [0, 255], or where it was sharpened
# img + (img - s) * 0.5 with img and the smoothed s both in [0, 255]: [-127.5, 382.5].  A coefficient of the
# forward transform of samples v is at most 64 * 0.4904^2 * max|v| = 15.4 * 382.5 < 5900 in magnitude before the DC's
# -1024: the rounded coefficient fits int16 with a wide margin (averaging only shrinks the samples).
PLANE_RANGE = (-127.5, 382.5)
FACTORS = [(fx, fy) for fx in (1, 2, 3, 4) for fy in (1, 2, 3, 4)]
# (no size here is a multiple of 8 * 3 in both directions; (3, 1): w < fx = 4; (45, 1): a single row)
PLANE_SIZES = FREE_SIZES + [(3, 1), (45, 1), (17, 17), (24, 9), (65, 9), (45, 37)]


def plane_cases(w, h):
    """frame_setds_source_x_clamped / _y_clamped / _inside: seeded samples over PLANE_RANGE, and a ramp."""
    rng = np.random.default_rng(SEED + 3 + 31 * w + h)
    lo, hi = PLANE_RANGE
    yield "noise", (lo + (hi - lo) * rng.random((h, w))).astype(np.float32)
    y, x = np.mgrid[0:h, 0:w]
    yield "ramp", (lo + (hi - lo) * ((3 * x + 5 * y) % 64) / 63.0).astype(np.float32)


def constant_planes():
    """Constant planes at 128 +- 1/16 and 128 +- 3/16: with an exact basis the DC would be 8 * 128.0625 - 1024 = 0.5, a
    rounding tie.  The reference's basis has ten decimal digits (0.3535533906^2 * 8 = 1 + 3.8e-11), so the DC lands
    4e-8 beside the tie, on the side the sign of the error decides: the nearest a plain constant comes."""
    for v in (128 + 1 / 16, 128 - 1 / 16, 128 + 3 / 16, 128 - 3 / 16):
        yield f"constant/{v}", np.full((16, 16), v, np.float32)


def _dc_of(block):
    return oracle.dct_double(block.astype(np.float64).reshape(64), inverse=False)[0] - 1024.0


def tie_block(target):
    """frame_setds_round_tie_positive / _negative: an 8x8 block of floats whose DC after the reference's forward
    transform is exactly `target` (+-0.5, +-1.5).  The DC is a sum of positive multiples of the samples, rounded to
    double after every term: monotone in every sample.  61 samples are 130, one makes up the sum 8 * (target + 1024)
    but for 0.1875, and two are bisected to the smallest value at which the DC reaches the target: the first over the
    floats around 0.1875 (steps of 2^-26: 2e-9 in the DC), then, one step back, the second over the floats up to
    2^-19 (steps of 2^-43 and less: below the DC's own spacing of 2^-42 beside 1024)."""
    blk = np.full(64, 130.0, np.float32)
    blk[2] = np.float32(8.0 * (target + 1024.0) - 61 * 130.0 - 0.1875)
    assert float(blk[2]) == 8.0 * (target + 1024.0) - 61 * 130.0 - 0.1875 and PLANE_RANGE[0] <= blk[2] <= PLANE_RANGE[1]
    blk[0], blk[1] = 0.1875, 0.0

    def bisect(i, lo, hi):
        # floats as integers: the order of positive floats is the order of their bit patterns
        a, b = int(np.float32(lo).view(np.uint32)), int(np.float32(hi).view(np.uint32))
        while a < b:
            m = (a + b) // 2
            blk[i] = np.uint32(m).view(np.float32)
            if _dc_of(blk) >= target:
                b = m
            else:
                a = m + 1
        return np.uint32(a).view(np.float32)

    blk[0] = bisect(0, 0.125, 0.25)
    blk[0] = np.uint32(int(blk[0].view(np.uint32)) - 1).view(np.float32)
    blk[1] = bisect(1, 2.0 ** -60, 2.0 ** -19)
    return blk.reshape(8, 8)


def tie_planes():
    """(name, plane, fx, fy): the tie blocks as they are, and each sample repeated 2 x 2 under a 2 x 2 average (the sum
    of four equal floats and its quarter are exact)."""
    for t in (0.5, -0.5, 1.5, -1.5):
        b = tie_block(t)
        yield f"tie/{t}/1x1", b, 1, 1
        yield f"tie/{t}/2x2", np.ascontiguousarray(np.repeat(np.repeat(b, 2, axis=0), 2, axis=1)), 2, 2


# -------------------------------------------------------------------------- YUV fields --
class Region(typing.NamedTuple):
    y: float
    u: float
    v: float
    what: str


# Normalised values as PreProcessChannel sees them (y in [0, 1], u and v in [-0.5, 0.5]); pass 1 is channel 2 (v),
# pass 2 channel 1 (u).
REGIONS = (
    Region(0.30, -0.10, 0.30, "dark and red in pass 1: v sharpened; pass 2: dark, not red, v >= -0.162 u"),
    Region(0.30, 0.30, 0.00, "dark and red in pass 2: u sharpened; pass 1: dark, not red, v >= -0.162 u"),
    Region(0.30, -0.10, -0.10, "dark, red in neither pass, v < -0.162 u: blurred where smooth, in both passes"),
    Region(0.95, 0.00, 0.00, "bright: dark in neither pass, nothing changes"),
    Region(0.30, 0.00, 0.10, "dark, red in neither pass, v >= -0.162 u: unchanged"),
    Region(0.88, 0.00, 0.00, "between the thresholds: r, g, b = 0.88 is not dark in pass 1 (g < 0.85 fails) nor in pass 2"),
    Region(0.86, -0.02, 0.02, "pass 1: g = 0.853, not dark; pass 2: r = 0.888, not dark; b = 0.825"),
    Region(0.80, 0.05, 0.06, "pass 1: r = 0.884 < 0.9 dark; pass 2: r = 0.884 >= 0.85 not dark: the two passes' dark tests differ"),
)
# A sample of magnitude |IMPULSE - 128| / 255 = 129 in a border pixel: there the edge image keeps the channel's value
# (Convolve2D leaves the border), which is then not below either threshold (0.02 * 127.5 and 127.5).
IMPULSE = -32767.0


def yuv_planes(w, h, variant):
    """Three float planes [h][w] in pixel units (0..255 but for the impulses)."""
    rng = np.random.default_rng(SEED + 4 + 31 * w + h + 1000 * variant)
    cell = (7, 5, 3)[variant % 3]
    gy, gx = -(-h // cell), -(-w // cell)
    types = rng.integers(0, len(REGIONS), (gy, gx))
    t = np.repeat(np.repeat(types, cell, axis=0), cell, axis=1)[:h, :w].copy()
    # isolated single pixels and 3x3 islands of another type: erode / dilate act on them or not; some in the border
    # row / column (which morph leaves alone) and in the two-pixel border of the convolutions
    for _ in range(max(2, w * h // 40)):
        x, y, s = int(rng.integers(0, w)), int(rng.integers(0, h)), int(rng.choice([1, 3]))
        t[y:y + s, x:x + s] = rng.integers(0, len(REGIONS))
    for x, y in ((0, 0), (w - 1, 0), (1, h - 1), (w - 2, 1), (0, h // 2)):
        t[y, x] = (t[y, x] + 1 + int(rng.integers(0, len(REGIONS) - 1))) % len(REGIONS)
    reg = np.array([(r.y, r.u, r.v) for r in REGIONS], np.float64)
    yuv = reg[t].transpose(2, 0, 1).copy()
    # soft edges: a triangle wave of +-0.02 across the cells (hard edges are the cell borders); integers and one
    # division, so that the planes are the same floats wherever they are made
    yy, xx = np.mgrid[0:h, 0:w]
    rip = 0.02 * (np.abs((2 * xx + 3 * yy + variant) % 12 - 6) / 3.0 - 1.0)
    yuv[1] += rip
    yuv[2] -= rip
    px = np.stack([yuv[0] * 255.0, (yuv[1] + 0.5) * 255.0, (yuv[2] + 0.5) * 255.0])
    if variant == 2:
        # the impulses: dark (y far below), not red, in border pixels: (0, 0) for pass 1 (v), (5, 0) for pass 2 (u)
        px[0, 0, 0] = px[0, 0, 5] = IMPULSE
        px[2, 0, 0] = IMPULSE
        px[1, 0, 5] = IMPULSE
    return px.astype(np.float32)


YUV_VARIANTS = (0, 1, 2)


def yuv_cases(w, h):
    """(name, 4:4:4 coefficients): the forward transform (SetDownsampledCoefficients with factors 1 x 1) of the field's
    planes, so that ToFloatPixels gives the field back to within the rounding of the coefficients."""
    for variant in YUV_VARIANTS:
        px = yuv_planes(w, h, variant)
        co = np.stack([oracle.set_downsampled(px[c], 1, 1) for c in range(3)])
        yield f"yuv/{variant}", co


def mixed_coeffs(w, h):
    """4:4:4 coefficients that walk a bank of every synthetic family's blocks (sparse, matrix rows, wrap, DC ramp, extreme
    chroma and luma), each component from another place in it: for the frames of thousands of blocks."""
    rng = np.random.default_rng(SEED + 5)
    bank = np.concatenate([np.stack([_sparse(p) for p in range(512)]), np.stack([_matrix_rows(p) for p in range(256)]),
                           np.stack([_wrap(p, rng) for p in range(256)]), np.stack([_dc_ramp(p) for p in range(97)]),
                           _extreme_chroma(64, 1, rng, False), _extreme_chroma(64, 0, rng, True)]).astype(np.int16)
    nb = grid(w, h)[2]
    i = np.arange(nb)
    return np.stack([bank[(7 * i + 389 * c) % len(bank)] for c in range(3)])
