"""Synthetic value-domain fields for the butteraugli chain: deterministic, file-free (but for the
photograph crop), fixed seeds.  The parity tests' usual input -- a photograph against a mildly
quantised copy of itself -- leaves most per-pixel value branches of the chain to luck; these
originals and candidates are chosen so that every reachable arm is taken by at least a wavefront
of samples (the oracle's branch census checks that: tests/test_value_domain.py).

`originals(w, h)` gives uint8 [h][w][3] images; `candidates(rgb)` gives, for one original, float32
[3][h][w] LINEAR planes in [0, 255] (what gz_probe_opsin / gz_probe_diffmap take); `pairs(w, h)`
walks every (original, candidate) pair as linear planes.

`search_cases(w, h)` / `search_cases_420(w, h)` are the inputs of phase A, the block search: an original image, the
coefficients the ranking reads, the candidate's coefficients, a target and the search's parameters."""
import typing

import numpy as np

import images
from checkers import oracle

SEED = 20261017


def _grey(v):
    return np.repeat(np.asarray(v, np.uint8)[:, :, None], 3, axis=2)


def checker(w, h, cell):
    y, x = np.mgrid[0:h, 0:w]
    return _grey(255 * (((x // cell) + (y // cell)) & 1))


def flat(w, h, v):
    return _grey(np.full((h, w), v))


def step_vertical(w, h):
    """Dark left, bright right; the edge at a column off the 8-, 16-, 32- and 64-pixel grids."""
    x = np.arange(w)[None, :].repeat(h, 0)
    edge = (w // 2) | 1    # odd
    return _grey(np.where(x < edge, 16, 235))


def step_horizontal(w, h):
    y = np.arange(h)[:, None].repeat(w, 1)
    edge = (h // 2) | 1
    return _grey(np.where(y < edge, 235, 16))


def ramp(w, h):
    x = np.arange(w, dtype=np.float64)[None, :]
    y = np.arange(h, dtype=np.float64)[:, None]
    r = 255.0 * x / max(w - 1, 1) + 0 * y
    g = 255.0 * y / max(h - 1, 1) + 0 * x
    b = 255.0 * (x + y) / max(w + h - 2, 1)
    return np.ascontiguousarray(np.stack([r, g, b], -1).astype(np.uint8))


def primaries(w, h, period=13):
    """Bars of the saturated corner colours of the RGB cube, 13 pixels wide: every bar edge falls
    inside a block, and X (red against green) swings to both of its extremes."""
    return images.stripes(w, h, period)


def impulses(w, h, background):
    """One full-scale pixel in about every 150, on a flat background."""
    rng = np.random.default_rng(SEED + background)
    v = np.full((h, w, 3), background, np.uint8)
    hit = rng.random((h, w)) < 1.0 / 150.0
    v[hit] = 255 - background
    return v


def discs(w, h, radius=3.3, pitch=16, inside=255, outside=0):
    """Small discs on a flat background, one every 16 pixels.  A blob about as wide as the HF
    filter's passband gives the largest |HF-Y| an image in [0, 255] reaches: bright discs on black
    cross maximum_clamp's upper bound on HF-Y (78.8), which checkers, steps and single pixels stay
    well below."""
    y, x = np.mgrid[0:h, 0:w]
    dx = (x % pitch) - pitch // 2
    dy = (y % pitch) - pitch // 2
    return _grey(np.where(dx * dx + dy * dy <= radius * radius, inside, outside))


def noise(w, h):
    return images.noise(w, h, seed=7)


def photo_with_zero_rectangle(w, h):
    """A photograph crop with a flat black rectangle over its middle, wider than twice the reach of
    the band filters: inside it every band plane of the original and of a block-coded candidate is
    exactly zero, so wavefronts and Malta tiles along its rim mix zero and non-zero samples."""
    rgb = images.crop(w, h, 0, 0).copy()
    rw, rh = (w * 5) // 8, (h * 3) // 4
    x0, y0 = (w - rw) // 2 + 3, (h - rh) // 2 + 1
    rgb[y0:y0 + rh, x0:x0 + rw] = 0
    return rgb


def originals(w, h):
    return {
        "checker1": checker(w, h, 1),
        "checker8": checker(w, h, 8),
        "black": flat(w, h, 0),
        "white": flat(w, h, 255),
        "grey": flat(w, h, 128),
        "step_v": step_vertical(w, h),
        "step_h": step_horizontal(w, h),
        "ramp": ramp(w, h),
        "primaries": primaries(w, h),
        "impulses_black": impulses(w, h, 0),
        "impulses_white": impulses(w, h, 255),
        "noise": noise(w, h),
        "discs": discs(w, h),
        "photo_zero_rect": photo_with_zero_rectangle(w, h),
    }


def linear(rgb):
    """uint8 [h][w][3] -> float32 [3][h][w] through the reference's sRGB table."""
    lut = oracle.srgb_table()
    return np.ascontiguousarray(lut[rgb].astype(np.float32).transpose(2, 0, 1))


def coded(rgb, qscale=6):
    """The linear planes of the image after a JPEG round trip with every quantiser = qscale."""
    h, w, _ = rgb.shape
    co = oracle.encode_rgb(rgb)
    _, _, lin1 = oracle.reconstruct(co, w, h, np.full((3, 64), qscale, np.int32))
    return lin1


def candidates(rgb):
    lin0 = linear(rgb)
    err = coded(rgb).astype(np.float64) - lin0
    return {
        "self": lin0.copy(),
        "inverse": (np.float32(255.0) - lin0).astype(np.float32),
        "flat": np.full_like(lin0, 117.25),
        "jpeg_error_x3": np.clip(lin0 + 3.0 * err, 0.0, 255.0).astype(np.float32),
        "jpeg_error_x10": np.clip(lin0 + 10.0 * err, 0.0, 255.0).astype(np.float32),
        "shift": np.ascontiguousarray(np.roll(lin0, 1, axis=2)),
        # values between the table's entries (the sRGB table has 256 of them)
        "off_table": (lin0 * np.float32(0.731) + np.float32(13.37)).astype(np.float32),
    }


def pairs(w, h, only=None):
    """(name, uint8 original, linear original, linear candidate) for every pair."""
    for oname, rgb in originals(w, h).items():
        if only is not None and oname not in only:
            continue
        lin0 = linear(rgb)
        for cname, lin1 in candidates(rgb).items():
            yield f"{oname}/{cname}", rgb, lin0, lin1


# ------------------------------------------------------------ phase A: the block search --
# Inputs of gz_block_zeroing_orders[_masked] beyond a photograph against its mildly quantised copy
# (tests/test_search_domain.py counts, with the oracle's search census, which arms of the search each
# family takes).  Coefficient arrays come from the oracle's encode_rgb / reconstruct.
class SearchCase(typing.NamedTuple):
    name: str
    rgb: np.ndarray        # uint8 [h][w][3]: the context's original image
    orig: np.ndarray       # int16: what the ranking scores read (gz_set_orig_coeffs where it is not rgb's own)
    cand: np.ndarray       # int16: the candidate the search starts from (gz_set_coeffs)
    target: float
    lookahead: int = 3
    new_model: bool = True
    comp_mask: int = 7
    foreign: bool = False  # orig is not what the library derives from rgb (gz_encode_rgb, gz_downsample)


TARGET = 0.971769
# The largest coefficient magnitude the search cases use: the whole int16 range, 32767 and -32768.  The reference's
# integer IDCT sums eight products of a coefficient with a constant of up to 11363 in an int, so from eight
# coefficients of about 2^15 on the sum passes 2^31, which C++ leaves undefined.  As compiled here the oracle and
# the unmodified reference both wrap, and they agree bit for bit on every case below at this magnitude (checked at
# 2^15, 2^14 and 2^13; tests/test_oracle_vs_ref.py::test_search_domain_oracle_equals_reference keeps checking it
# where oracle/_ref is built), so nothing was shrunk.  Should a compiler make the two disagree, this is the bound to
# lower, to the largest power of two at which they agree again.
EXTREME = 1 << 15


def _quantised(co, w, h, q):
    return oracle.reconstruct(co, w, h, np.broadcast_to(np.asarray(q, np.int32), (3, 64)).copy())[0]


def extremes(co, mag=EXTREME):
    """mag - 1 or -mag in every AC position of every third block, the signs by position; the other blocks are co's.
    mag = EXTREME = 2^15 is the bound up to which the oracle and the unmodified reference agree (the note above)."""
    out = co.copy()
    k = np.arange(64)
    val = np.where(((k & 7) + (k >> 3)) & 1, -(mag - 1), mag - 1)
    val[k % 5 == 0] = -mag
    val = val.astype(np.int16)
    out[:, ::3, 1:] = val[1:]
    return out


def sparse_wide(co, rng, mag=EXTREME):
    """Uniform over [-mag, mag) with 60 % zeros (DC included: a DC far outside [0, 255] saturates whole blocks)."""
    out = rng.integers(-mag, mag, size=co.shape).astype(np.int16)
    out[rng.random(co.shape) < 0.6] = 0
    return out


def matrix_quantiser():
    """A per-coefficient quantiser as parity_cases.case_jpeg_entropy draws one: luma 1..8, chroma 1..29."""
    rng = np.random.default_rng(SEED + 31)
    return np.stack([rng.integers(1, 9, 64), rng.integers(1, 30, 64), rng.integers(1, 30, 64)]).astype(np.int32)


def search_originals(w, h):
    import parity_cases
    o = originals(w, h)
    o["colourful"] = parity_cases.colourful(w, h)
    return o


def search_cases(w, h, only=None):
    """SearchCase tuples for a 4:4:4 frame of w x h; `only`: the families to walk (the part of the name before the
    first slash)."""
    def want(family):
        return only is None or family in only
    imgs = search_originals(w, h)
    co = {}

    def coeffs(name):
        if name not in co:
            co[name] = oracle.encode_rgb(imgs[name])
        return co[name]

    if want("field"):
        for name, rgb in imgs.items():
            yield SearchCase(f"field/{name}", rgb, coeffs(name), _quantised(coeffs(name), w, h, 2), TARGET)
    if want("target"):
        for t in (0.3, 3.0):
            yield SearchCase(f"target/noise/{t}", imgs["noise"], coeffs("noise"), coeffs("noise").copy(), t)
    if want("zero_error"):
        rng = np.random.default_rng(5)
        for name in ("white", "black", "grey"):
            cand = coeffs(name).copy()
            hit = rng.random(cand.shape) < 0.05
            hit[:, :, 0] = False
            tiny = (rng.integers(1, 4, cand.shape) * rng.choice([-1, 1], cand.shape)).astype(np.int16)
            cand[hit] = tiny[hit]
            yield SearchCase(f"zero_error/{name}", imgs[name], coeffs(name), cand, TARGET)
    photo, pco = imgs["photo_zero_rect"], None
    if want("saturating") or want("foreign_orig") or want("matrix"):
        pco = coeffs("photo_zero_rect")
    if want("saturating"):
        x4 = np.clip(pco.astype(np.int32) * 4, -32768, 32767).astype(np.int16)
        yield SearchCase("saturating/x4", photo, pco, x4, TARGET)
        rng = np.random.default_rng(SEED + 2040)
        wild = rng.integers(-2040, 2041, size=pco.shape).astype(np.int16)
        for t in (50.0, 500.0):
            yield SearchCase(f"saturating/uniform2040/{t}", photo, pco, wild, t)
        yield SearchCase("saturating/extremes/500.0", photo, pco, extremes(pco), 500.0)
        sw = sparse_wide(pco, np.random.default_rng(SEED + 16384))
        for t in (50.0, 500.0):
            yield SearchCase(f"saturating/sparse_wide/{t}", photo, pco, sw, t)
    if want("foreign_orig"):
        cand = _quantised(pco, w, h, 2)
        yield SearchCase("foreign_orig/noise", photo, coeffs("noise"), cand, TARGET, foreign=True)
        ext = extremes(pco)   # (as orig it is only scored, abs(-32768) included, never transformed)
        yield SearchCase("foreign_orig/extremes", photo, ext, cand, TARGET, foreign=True)
        yield SearchCase("foreign_orig/extremes/old_model", photo, ext, cand, TARGET, new_model=False, foreign=True)
    if want("matrix"):
        yield SearchCase("matrix/photo_zero_rect", photo, pco, _quantised(pco, w, h, matrix_quantiser()), TARGET)
    if want("params"):
        for name in ("noise", "discs", "primaries", "checker1"):
            cand = _quantised(coeffs(name), w, h, 2)
            for mask in (1, 6):
                yield SearchCase(f"params/{name}/mask{mask}", imgs[name], coeffs(name), cand, TARGET, comp_mask=mask)
            yield SearchCase(f"params/{name}/lookahead5/old_model", imgs[name], coeffs(name), cand, TARGET,
                             lookahead=5, new_model=False)
        cand = _quantised(coeffs("noise"), w, h, 2)
        for la in (1, 7):   # (7 is no multiple of the kernel's batch of three: the last batch is partial)
            yield SearchCase(f"params/noise/lookahead{la}", imgs["noise"], coeffs("noise"), cand, TARGET, lookahead=la)


SEARCH_FIELDS_420 = ("ramp", "primaries", "noise", "colourful", "photo_zero_rect")


def search_cases_420(w, h, only=None):
    """SearchCase tuples on the 4:2:0 frame of w x h (orig = the oracle's downsample of the original, cand = its
    quantised coefficients; frame layout: luma blocks, Cb, Cr), component masks 1 and 6.  Grey fields have no
    chroma candidates and appear under mask 1 only."""
    imgs = search_originals(w, h)
    nb = ((w + 7) // 8) * ((h + 7) // 8)
    for name in SEARCH_FIELDS_420:
        if only is not None and name not in only:
            continue
        orig = oracle.downsample(oracle.encode_rgb(imgs[name]), w, h)
        cand = oracle.reconstruct420(orig, w, h, np.full((3, 64), 2, np.int32))[0]
        for t in (TARGET, 3.0):
            for mask in (1, 6):
                yield SearchCase(f"420/{name}/{t}/mask{mask}", imgs[name], orig, cand, t, comp_mask=mask)
    if only is None or "white" in only:
        # (the reference leaves a grey image's frame 4:4:4: its 4:2:0 frame is put together here, chroma all zero,
        #  and goes in through gz_set_orig_coeffs_420)
        nbc = ((w + 15) // 16) * ((h + 15) // 16)
        orig = np.concatenate([oracle.encode_rgb(imgs["white"])[0], np.zeros((2 * nbc, 64), np.int16)])
        rng = np.random.default_rng(5)
        cand = orig.copy()
        hit = rng.random(cand.shape) < 0.05
        hit[:, 0] = False
        hit[nb:] = False
        tiny = (rng.integers(1, 4, cand.shape) * rng.choice([-1, 1], cand.shape)).astype(np.int16)
        cand[hit] = tiny[hit]
        yield SearchCase("420/white/tiny_ac/mask1", imgs["white"], orig, cand, TARGET, comp_mask=1, foreign=True)
