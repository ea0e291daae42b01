"""Synthetic value-domain fields for the butteraugli chain: deterministic, file-free (but for the
photograph crop), fixed seeds.  The parity tests' usual input -- a photograph against a mildly
quantised copy of itself -- leaves most per-pixel value branches of the chain to luck; these
originals and candidates are chosen so that every reachable arm is taken by at least a wavefront
of samples (the oracle's branch census checks that: tests/test_value_domain.py).

`originals(w, h)` gives uint8 [h][w][3] images; `candidates(rgb)` gives, for one original, float32
[3][h][w] LINEAR planes in [0, 255] (what gz_probe_opsin / gz_probe_diffmap take); `pairs(w, h)`
walks every (original, candidate) pair as linear planes."""
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
