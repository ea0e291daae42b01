"""CPU: which arm of which value branch of the frame path (pixels -> coefficients -> pixels: quantisation, the integer
IDCT and the colour transform of both reconstructions, EncodeRGBToJpeg's edge replication, the 4:2:0 upsampler,
SetDownsampledCoefficients, PreProcessChannel) the families of tests/frame_domain.py take, counted by the oracle's frame_*
census (test infrastructure, independent of the kernels), at the sizes tests/test_frame_gpu.py runs them at.

Every arm must be taken by at least one named case, or be listed in UNREACHED with the reason.  The counts are recorded in
tests/golden/frame_census.json beside what the photograph cases of the GPU suite reach (case_downsample_component,
case_encode_quantize_reconstruct, case_frame420 and its `colourful` picture), and re-derived here.
(`python tests/test_frame_domain.py --write` regenerates the file.)

The same cases run here through the emulation library, and, where oracle/_ref is built, the oracle itself is pinned on
them against the unmodified reference wherever that exposes the stage."""
import json
import os
import sys

import numpy as np
import pytest

import frame_domain as fd
import images
import parity_cases as pc
from checkers import assert_bits_equal, oracle, ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "frame_census.json")
needs_ref = pytest.mark.skipif(ref is None, reason="oracle/_ref/libgz_ref.so not built")

# Arms no case takes, with the reason.  A case that does take one makes the test below fail as a stale entry.
UNREACHED = {}

ENCODE_SIZES = fd.PIXEL_SIZES + fd.FREE_SIZES + fd.CTX_SIZES[:9]
EMU_STRIP_SIZES = [(139, 24), (272, 16)]


def _counted(f, *a, **k):
    oracle.census_reset()
    f(*a, **k)
    return oracle.frame_census()


def _add(per_case, name, census):
    dst = per_case.setdefault(name, {a: 0 for a in census})
    for a, v in census.items():
        dst[a] += v


def family_census():
    """{case name: census}: every family walked as the case functions of tests/parity_cases.py walk it, the counts of
    a name summed over the sizes."""
    out = {}
    for w, h in fd.CTX_SIZES:
        for layout, rec in (("444", oracle.reconstruct), ("420", oracle.reconstruct420)):
            for family, co in fd.coeff_cases(w, h, layout):
                for qn, q in fd.quant_tables(co, layout, w, h):
                    _add(out, f"coeffs{layout}/{family}/{qn}", _counted(rec, co, w, h, q))
        for name, co in pc.frame_downsample_inputs(w, h):
            _add(out, f"downsample/{name}", _counted(oracle.downsample, co, w, h))
    _add(out, "encode/lattice", _counted(oracle.encode_rgb, fd.lattice_image()))
    for w, h in ENCODE_SIZES:
        for name, rgb in fd.pixel_cases(w, h):
            _add(out, f"encode/{name}", _counted(oracle.encode_rgb, rgb))
    for w, h in fd.PLANE_SIZES:
        for name, p in fd.plane_cases(w, h):
            for fx, fy in fd.FACTORS:
                _add(out, f"planes/{name}", _counted(oracle.set_downsampled, p, fx, fy))
    for name, p, fx, fy in fd.tie_planes():
        _add(out, f"planes/{name}", _counted(oracle.set_downsampled, p, fx, fy))
    for name, p in fd.constant_planes():
        for fx, fy in ((1, 1), (2, 2)):
            _add(out, "planes/constant", _counted(oracle.set_downsampled, p, fx, fy))
    return out


def bees_census():
    """The oracle calls of the frame path's photograph cases in tests/test_gpu_parity.py, at its sizes."""
    out = {}
    for w, h in ((444, 258), (61, 43), (32, 32), (8, 8), (129, 9), (1, 1)):       # case_downsample_component
        def walk():
            co = oracle.encode_rgb(images.crop(w, h, 0, 0))
            for c in range(3):
                oracle.to_float_pixels(co[c], w, h)
            for fx, fy in ((2, 2), (1, 1)):
                oracle.downsample_chroma(co, w, h, fx, fy)
        _add(out, "case_downsample_component", _counted(walk))
    for w, h in ((444, 258), (61, 43), (32, 32), (8, 8), (129, 9)):               # case_encode_quantize_reconstruct
        def walk():
            rng = np.random.default_rng(pc.RNG_SEED + w)
            co = oracle.encode_rgb(images.crop(w, h, 0, 0))
            q = np.stack([rng.integers(1, 12, size=64), rng.integers(1, 20, size=64),
                          rng.integers(1, 20, size=64)]).astype(np.int32)
            for qq in (None, q):
                oracle.reconstruct(co, w, h, qq)
        _add(out, "case_encode_quantize_reconstruct", _counted(walk))

    def frame420(rgb, w, h):
        rng = np.random.default_rng(pc.RNG_SEED + 11 * w + h)
        exp = oracle.downsample(oracle.encode_rgb(rgb), w, h)
        q = np.stack([rng.integers(1, 8, 64), rng.integers(1, 12, 64), rng.integers(1, 12, 64)]).astype(np.int32)
        for qq in (None, q):
            oracle.reconstruct420(exp, w, h, qq, shuffle=7)
    for w, h in ((48, 40), (33, 35), (47, 31), (444, 258), (129, 70)):            # case_frame420
        _add(out, "case_frame420", _counted(frame420, images.crop(w, h, 0, 0), w, h))
    _add(out, "colourful", _counted(frame420, pc.colourful(200, 136), 200, 136))
    return out


def _merged(per_case):
    arms = sorted(oracle.frame_census())
    out = {}
    for a in arms:
        best = max(per_case, key=lambda n: per_case[n][a])
        out[a] = {"count": sum(c[a] for c in per_case.values()), "most_on": best if per_case[best][a] else ""}
    return out


def derive():
    fam, bees = family_census(), bees_census()
    mf, mb = _merged(fam), _merged(bees)
    return {
        "arms": sorted(oracle.frame_census()),
        "sizes": ["%dx%d" % s for s in fd.CTX_SIZES],
        "bees_cases": mb,
        "family_cases": mf,
        "arms_reached": {"bees_cases": sum(v["count"] > 0 for v in mb.values()),
                         "family_cases": sum(v["count"] > 0 for v in mf.values()), "of": len(mf)},
        "per_bees_case": {n: {a: v for a, v in c.items() if v} for n, c in bees.items()},
        "per_family_case": {n: {a: v for a, v in c.items() if v} for n, c in fam.items()},
    }


_derived = None


def derived():
    global _derived
    if _derived is None:
        _derived = derive()
    return _derived


def test_families_take_every_arm_or_it_is_listed():
    d = derived()
    assert len(d["arms"]) >= 70
    assert set(UNREACHED) <= set(d["arms"]), "an arm listed as unreached does not exist"
    missed = [a for a in d["arms"] if d["family_cases"][a]["count"] == 0 and a not in UNREACHED]
    assert not missed, f"arms no family takes: {missed}"
    stale = [a for a in UNREACHED if d["family_cases"][a]["count"] > 0]
    assert not stale, stale
    for a in d["arms"]:   # reached means: by a case with a name
        assert (d["family_cases"][a]["most_on"] != "") == (d["family_cases"][a]["count"] > 0)


def test_census_equals_the_recorded_one():
    """tests/golden/frame_census.json is the record of the gap: per arm, what the photograph cases reach beside what the
    families reach."""
    rec = json.load(open(GOLDEN))
    assert derived() == rec
    gap = [a for a in rec["arms"] if rec["family_cases"][a]["count"] > 0 and rec["bees_cases"][a]["count"] == 0]
    assert gap, "the photograph cases reach every arm the families reach: nothing recorded to close"


def test_families_meet_their_conditions():
    """What each family is in the set for, so that a change to a generator that empties it fails here."""
    per = derived()["per_family_case"]

    def n(case, arm):
        return per[case].get(arm, 0)
    # quantiser tables: ties of both signs and the int16 wrap come from the tables built for them
    for layout in ("444", "420"):
        assert n(f"coeffs{layout}/sparse/ties", "frame_quant_tie_positive") > 0
        assert n(f"coeffs{layout}/sparse/ties", "frame_quant_tie_negative") > 0
        assert n(f"coeffs{layout}/wrap/ties", "frame_quant_round_up") > 0 and n(f"coeffs{layout}/wrap/ties", "frame_quant_round_down") > 0
        assert n(f"coeffs{layout}/wrap/large", "frame_quant_wrapped_int16") > 0
        assert n(f"coeffs{layout}/wrap/large", "frame_quant_q_above_raw") > 0
        assert n(f"coeffs{layout}/photo/ones", "frame_quant_round_up") == 0
        # the IDCT: the column pass leaves int16 on sparse, matrix_rows and wrap, and never on the photograph
        for family in ("sparse", "matrix_rows", "wrap"):
            assert n(f"coeffs{layout}/{family}/ones", "frame_idct_column_wraps_int16") > 0, family
        assert n(f"coeffs{layout}/photo/ones", "frame_idct_column_wraps_int16") == 0
        assert n(f"coeffs{layout}/dc_ramp/ones", "frame_idct_pixel_clamped_low") > 0
        assert n(f"coeffs{layout}/dc_ramp/ones", "frame_idct_pixel_clamped_high") > 0
        # the colour transform's clamps with the IDCT's pixels inside [0, 255]
        rgb = "frame_rgb%s_clamped_" % layout
        assert n(f"coeffs{layout}/chroma_extreme/ones", rgb + "low") > 0 and n(f"coeffs{layout}/chroma_extreme/ones", rgb + "high") > 0
    for side in ("left", "right", "top", "bottom"):
        assert n("coeffs420/chroma_extreme/ones", f"frame_up420_neighbour_clamped_{side}") > 0, side
    # SetDownsampledCoefficients: exact ties of both signs, each rounded away from zero (checked in case_frame_planes)
    for t in (0.5, 1.5):
        assert n(f"planes/tie/{t}/1x1", "frame_setds_round_tie_positive") == 1
        assert n(f"planes/tie/{-t}/2x2", "frame_setds_round_tie_negative") == 1
    assert n("planes/constant", "frame_setds_round_tie_positive") == 0      # (frame_domain.constant_planes says why)
    assert n("planes/noise", "frame_setds_source_x_clamped") > 0 and n("planes/noise", "frame_setds_source_y_clamped") > 0
    # PreProcessChannel: the impulse field alone takes a border pixel's |edge| to the thresholds, in both passes
    for p in ("pp2", "pp1"):
        assert n("downsample/yuv/2", f"frame_{p}_edge_not_below_threshold") > 0
        assert n("downsample/yuv/0", f"frame_{p}_edge_not_below_threshold") == 0
        for arm in ("out_sharpened", "out_blurred", "out_unchanged", "erode_clears", "erode_keeps", "dilate_sets", "dilate_keeps",
                    "v_below_scaled_u_true", "v_below_scaled_u_false", "conv_h_border", "conv_v_border"):
            assert n("downsample/yuv/0", f"frame_{p}_{arm}") > 0, (p, arm)
    # every family's sums stay inside int32 (the reference sums in int)
    for w, h in fd.CTX_SIZES:
        for layout in ("444", "420"):
            for family, co in fd.coeff_cases(w, h, layout):
                assert fd.idct_sums_fit_int32(co), (family, layout, w, h)
    assert fd.idct_sums_fit_int32(np.full((1, 64), -32768, np.int16)), "the bound holds for every int16 block"


def test_int64_idct_equals_the_oracle():
    """frame_domain.idct_blocks_int64, the evaluation the magnitude assertions rest on, is the oracle's IDCT."""
    blocks = np.concatenate([fd.luma_extreme_blocks(300), fd.mixed_coeffs(64, 64)[1]])
    px, bound, wrapped = fd.idct_blocks_int64(blocks)
    assert bound < (1 << 31) and wrapped > 0
    assert_bits_equal(px, np.stack([oracle.idct_block(b) for b in blocks]), "int64 IDCT")


# ------------------------------------------------------------- through the emulation library --
@pytest.fixture(scope="module")
def L():
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    from guetzli_amd.capi import Library
    return Library(build_emu.build())


@pytest.fixture(scope="module")
def contexts(L):
    cache = pc.TargetContexts(L)
    yield cache
    cache.close()


def test_emu_encode(L, contexts):
    pc.case_frame_encode(L, contexts, ENCODE_SIZES)


def test_emu_planes(L):
    pc.case_frame_planes(L)


def test_emu_free_sizes(L):
    pc.case_frame_free_sizes(L)


@pytest.mark.parametrize("wh", fd.CTX_SIZES)
def test_emu_coeffs444(L, contexts, wh):
    for family in fd.COEFF_FAMILIES:
        pc.case_frame_coeffs444(L, contexts, *wh, family)


@pytest.mark.parametrize("wh", fd.CTX_SIZES)
def test_emu_coeffs420(L, contexts, wh):
    for family in fd.COEFF_FAMILIES:
        pc.case_frame_coeffs420(L, contexts, *wh, family)


@pytest.mark.parametrize("wh", fd.CTX_SIZES)
def test_emu_downsample(L, contexts, wh):
    pc.case_frame_downsample(L, contexts, *wh)


@pytest.mark.parametrize("wh", fd.CTX_SIZES)
def test_emu_idct_copies(L, contexts, wh):
    pc.case_frame_idct_copies(L, contexts, *wh)


@pytest.mark.parametrize("strips", [2, 4])
@pytest.mark.parametrize("wh", EMU_STRIP_SIZES)
def test_emu_strip_loop(L, monkeypatch, wh, strips):
    """k_reconstruct's strip loop forced on frames the emulation can afford: (139, 24) three strips, the last with two
    live blocks, a row pitch that is no multiple of 4 (the scalar stores); (272, 16) five strips, pitch 272."""
    monkeypatch.setenv("GZ_EMU_RECON_STRIPS", str(strips))
    pc.case_frame_strips(L, *wh)


# ------------------------------------------------------- the oracle against the reference --
@needs_ref
@pytest.mark.parametrize("wh", fd.CTX_SIZES)
def test_oracle_equals_reference_on_coefficients(wh):
    w, h = wh
    for family in fd.COEFF_FAMILIES:
        for layout, name in (("444", "reconstruct"), ("420", "reconstruct420")):
            co = fd.coeffs_of(family, w, h, layout)
            for qn, q in fd.quant_tables(co, layout, w, h):
                for a, b, what in zip(getattr(oracle, name)(co, w, h, q), getattr(ref, name)(co, w, h, q),
                                      ("coefficients", "srgb", "linear")):
                    assert_bits_equal(a, b, f"{name} {what}: {family} q={qn} {w}x{h}")


@needs_ref
@pytest.mark.parametrize("wh", fd.CTX_SIZES)
def test_oracle_equals_reference_on_downsample(wh):
    w, h = wh
    for name, co in pc.frame_downsample_inputs(w, h):
        assert_bits_equal(oracle.downsample(co, w, h), ref.downsample(co, w, h), f"downsample {name} {w}x{h}")
        for c in range(3):
            assert_bits_equal(oracle.to_float_pixels(co[c], w, h), ref.to_float_pixels(co[c], w, h),
                              f"to_float_pixels {name} c={c} {w}x{h}")
        # (of the sixteen factor pairs the reference runs 2 x 2 alone: its Downsample leaves a 1 x 1 component's
        # coefficients as they are, and its pixel model leaves the process at any other pair)
        for fx, fy in ((2, 2),):
            for a, b in zip(oracle.downsample_chroma(co, w, h, fx, fy), ref.downsample_chroma(co, w, h, fx, fy)):
                assert_bits_equal(a, b, f"downsample_chroma {name} {w}x{h} by {fx}x{fy}")


@needs_ref
def test_oracle_equals_reference_on_pixels():
    img = fd.lattice_image()
    assert_bits_equal(oracle.encode_rgb(img), ref.encode_rgb(img), "encode_rgb lattice")
    for w, h in ENCODE_SIZES:
        for name, rgb in fd.pixel_cases(w, h):
            assert_bits_equal(oracle.encode_rgb(rgb), ref.encode_rgb(rgb), f"encode_rgb {name} {w}x{h}")
    for w, h in EMU_STRIP_SIZES:
        co = fd.mixed_coeffs(w, h)
        for a, b in zip(oracle.reconstruct(co, w, h), ref.reconstruct(co, w, h)):
            assert_bits_equal(a, b, f"reconstruct mixed {w}x{h}")


if __name__ == "__main__":
    if "--write" in sys.argv:
        json.dump(derive(), open(GOLDEN, "w"), indent=1, sort_keys=True)
        print("wrote", GOLDEN)
    else:
        print(json.dumps(derive(), indent=1, sort_keys=True))
