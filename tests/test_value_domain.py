"""CPU: which arm of which value branch of the butteraugli chain the parity tests' inputs take,
counted by the oracle (orc_branch_census: test infrastructure, independent of the kernels).

The synthetic fields of tests/fields.py, at the sizes the GPU suite runs them at, must take every
arm that is reachable by at least one wavefront (64 samples) on at least one field; the arms that
are not reachable are listed with the reason, and tests/cpp/test_device_math.cc evaluates the
per-pixel functions on them element-wise.  The counts are recorded in
tests/golden/value_domain_census.json beside what the photograph pairs of case_stages / case_compare
reach, and re-derived here.  (`python tests/test_value_domain.py --write` regenerates the file.)"""
import json
import os
import sys

import numpy as np

import fields
import parity_cases as pc
from checkers import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "value_domain_census.json")

GPU_SIZES = [(444, 258), (333, 141)]   # tests/test_gpu_parity.py: the value-domain cases
EMU_SIZE = (200, 110)                  # tests/test_kernels_emu.py: the interior-tile case
WAVEFRONT = 64

# Arms no input in [0, 255] takes.  Each is evaluated element-wise on the device by
# gz_probe_math (tests/cpp/test_device_math.cc) instead.
UNREACHABLE = {
    "gamma_yq_zero": "on the absorbances of [0, 255] inputs, 1.016 .. 217.8, the denominator polynomial of "
                     "GammaPolynomial stays between 3.2e-5 and 0.034: no root",
    "gamma_nonfinite": "absorbances of finite inputs are finite",
    "lut_index_negative": "the mask tables are indexed by blurs (positive weights) of sums of absolute "
                          "differences: never negative",
    "malta_sum_outside_2p100": "band samples of [0, 255] inputs are differences of blurs of values between 2^-5 and "
                               "2^10: exactly 0 (counted as malta_sum_zero) or a rounding residue of such values "
                               "at the least, tens of binary orders away from 2^-100 and 2^100",
    "malta_den_above_2p40": "the largest norm1 is 8.3e7 and band values stay below 2^10: the denominator "
                            "norm1 + absval is far below 2^40",
}
# Not proven unreachable, but no [0, 255] image found that takes them.  SameNoiseLevels clamps the finished HF-Y
# plane at 85.7; that plane has already been through maximum_clamp (78.8, the excess times 0.69).  The largest
# finished HF-Y found is 84.2: white discs of radius 3.0 to 3.5 on black (fields.discs).  Tried at 160x120: white
# and black discs of radius 2 to 5 at pitches 12, 16 and 24 on black, white and three greys; squares of 3 to 7
# pixels; checkers of 2 to 8 pixels.  The margin left is 1.5, so these two stay a finding of the search, not a
# proof: a field that does reach them makes the test below fail as a stale entry.
NOT_REACHED = {
    "same_noise_clamp0": "the largest finished HF-Y of any [0, 255] image tried is 84.2 (white discs of radius 3.3 "
                         "on black) against the clamp at 85.7",
    "same_noise_clamp1": "as same_noise_clamp0, for the candidate",
}
UNREACHABLE.update(NOT_REACHED)
# Reached only by the XYB planes scaled by +-40 that the stage probes are also given (parity_cases.XYB_SCALES), not
# by any [0, 255] image through probe_diffmap or the production compare.  maximum_clamp's lower arm needs HF-Y below
# -78.8 before the clamp; the opsin's compression of bright values leaves dark blobs on white less contrast than
# bright blobs on black: the most negative finished HF-Y found is -75.1 (black discs of radius 3.3 to 3.5 on white,
# pitch 16; radius 2 to 5, pitches 12 to 24 and black squares of 3 to 7 pixels were tried), where the white discs
# that take the upper arm reach +84.2.
ONLY_SCALED_XYB = ("hf_y_maximum_clamp_below", "lut_index_top")
# Taken by a plain [0, 255] image, whatever the scaled planes add: fields.discs is in the set for this arm.
ON_A_PLAIN_FIELD = ("hf_y_maximum_clamp_above",)
# (MaltaNorm::fast_div == 0 is no value branch: the host sets it per pass from the pass's constants, and all six
#  production normalisations set it to 1.  gz_probe_math passes a norm with fast_div = 0.)


def _merge(best, counts, name):
    for arm, n in counts.items():
        if n > best.get(arm, (0, ""))[0]:
            best[arm] = (n, name)


def field_census(sizes):
    """{arm: (largest count on one field, that field)} over the field pairs through the oracle's diffmap, the
    originals through its comparator at the cases' quantisers, and the scaled XYB planes through its
    separate_frequencies and mask; and the same over the [0, 255] images alone."""
    best, plain = {}, {}
    for w, h in sizes:
        for name, rgb, lin0, lin1 in fields.pairs(w, h):
            oracle.census_reset()
            oracle.diffmap(lin0, lin1)
            _merge(best, oracle.census(), f"{name} {w}x{h}")
            _merge(plain, oracle.census(), f"{name} {w}x{h}")
            if name.endswith(("/self", "/inverse")):
                x0, x1 = oracle.opsin(lin0), oracle.opsin(lin1)
                for s in pc.XYB_SCALES:
                    oracle.census_reset()
                    oracle.separate_frequencies(x1 * np.float32(s))
                    oracle.mask(x0 * np.float32(s), x1 * np.float32(s))
                    _merge(best, oracle.census(), f"{name} xyb x {s} {w}x{h}")
        for oname, rgb in fields.originals(w, h).items():
            oc = oracle.comparator(rgb, 0.971769)
            co = oracle.encode_rgb(rgb)
            for qs in pc.VALUE_DOMAIN_QSCALES:
                cq, _, _ = oracle.reconstruct(co, w, h, np.full((3, 64), qs, np.int32))
                oracle.census_reset()
                oc.compare(cq)
                _merge(best, oracle.census(), f"{oname} compare q={qs} {w}x{h}")
                _merge(plain, oracle.census(), f"{oname} compare q={qs} {w}x{h}")
            oc.close()
    return best, plain


def photograph_census():
    """The same for what the suite fed the chain before: case_stages' pair and case_compare's candidates of the
    444x258 photograph (tests/test_gpu_parity.py: test_stages, test_compare_bees)."""
    best = {}
    w, h = 444, 258
    rgb, co, cq, lin0, lin1 = pc._linear_pair(w, h, 0, 0, 6)
    oracle.census_reset()
    oracle.diffmap(lin0, lin1)
    _merge(best, oracle.census(), "case_stages 444x258")
    oc = oracle.comparator(rgb, 0.971769)
    for qs in (1, 2, 6, 14):
        cq, _, _ = oracle.reconstruct(co, w, h, np.full((3, 64), qs, np.int32))
        oracle.census_reset()
        oc.compare(cq)
        _merge(best, oracle.census(), f"case_compare q={qs} 444x258")
    oc.close()
    return best


def mixed_malta_tiles(lin0, lin1):
    """Per band plane Malta reads: the number of 64x32 Malta tiles that hold both sample pairs with
    |a| + |b| == 0 (malta_diff's rare path) and pairs without."""
    s0 = oracle.separate_frequencies(oracle.opsin(lin0))
    s1 = oracle.separate_frequencies(oracle.opsin(lin1))
    out = {}
    for nm, i in (("mf_x", 3), ("mf_y", 4), ("hf_x", 6), ("hf_y", 7), ("uhf_x", 8), ("uhf_y", 9)):
        zero = (np.abs(s0[i]) + np.abs(s1[i])) == 0
        h, w = zero.shape
        n = 0
        for y0 in range(0, h, 32):
            for x0 in range(0, w, 64):
                t = zero[y0:y0 + 32, x0:x0 + 64]
                n += bool(t.any() and not t.all())
        out[nm] = n
    return out


def mixed_tiles_of_the_rectangle_field(w, h):
    rgb = fields.photo_with_zero_rectangle(w, h)
    return mixed_malta_tiles(fields.linear(rgb), fields.candidates(rgb)["jpeg_error_x3"])


def as_json(best):
    return {arm: {"samples": n, "field": name} for arm, (n, name) in sorted(best.items())}


def derive():
    arms = sorted(oracle.census())
    (fc, plain), ph = field_census(GPU_SIZES), photograph_census()
    return {
        "arms": arms,
        "fields": as_json({a: fc.get(a, (0, "")) for a in arms}),
        "fields_without_scaled_xyb": as_json({a: plain.get(a, (0, "")) for a in arms}),
        "photograph_pairs": as_json({a: ph.get(a, (0, "")) for a in arms}),
        "mixed_malta_tiles": {f"{w}x{h}": mixed_tiles_of_the_rectangle_field(w, h) for w, h in [EMU_SIZE] + GPU_SIZES},
    }


_derived = None


def derived():
    global _derived
    if _derived is None:
        _derived = derive()
    return _derived


def test_fields_take_every_reachable_arm():
    d = derived()
    assert set(UNREACHABLE) <= set(d["arms"]), "an arm listed as unreachable does not exist"
    short = {a: v for a, v in d["fields"].items() if v["samples"] < WAVEFRONT and a not in UNREACHABLE}
    assert not short, f"arms taken by fewer than {WAVEFRONT} samples on every field: {short}"
    # an arm listed as unreachable that a field does reach is a stale entry
    stale = [a for a in UNREACHABLE if d["fields"][a]["samples"] > 0]
    assert not stale, stale
    plain = d["fields_without_scaled_xyb"]
    for a in ONLY_SCALED_XYB:
        assert plain[a]["samples"] == 0, f"{a} is listed as scaled-only but a [0, 255] image takes it: {plain[a]}"
    # every other reachable arm by a wavefront on a [0, 255] image: through gz_probe_diffmap or the production compare
    short = {a: v for a, v in plain.items()
             if v["samples"] < WAVEFRONT and a not in UNREACHABLE and a not in ONLY_SCALED_XYB}
    assert not short, f"arms no [0, 255] image takes by {WAVEFRONT} samples: {short}"
    for a in ON_A_PLAIN_FIELD:
        assert plain[a]["samples"] >= WAVEFRONT, (a, plain[a])


def test_rectangle_field_mixes_zero_and_nonzero_pairs_in_malta_tiles():
    """malta_diff's rare path (|a| + |b| == 0) beside the normal one inside one tile, hence inside
    wavefronts: at least one tile at the emulation's size, eight at the GPU's, on each plane of the two
    highest bands and on MF-X.  (MF-Y is never exactly zero: amplify_range doubles the rounding residue
    of the LF blur of a flat region, which is not zero.)"""
    d = derived()["mixed_malta_tiles"]
    for plane in ("uhf_x", "uhf_y", "hf_x", "hf_y", "mf_x"):
        assert d["%dx%d" % EMU_SIZE][plane] >= 1, (plane, d)
        assert d["%dx%d" % GPU_SIZES[0]][plane] >= 8, (plane, d)


def test_census_equals_the_recorded_one():
    """tests/golden/value_domain_census.json is the record of the gap: what the photograph pairs reach
    beside what the fields reach."""
    rec = json.load(open(GOLDEN))
    assert derived() == rec
    # the gap on record: arms the fields take by a wavefront that the photograph pairs do not
    gap = [a for a in rec["arms"] if rec["fields"][a]["samples"] >= WAVEFRONT > rec["photograph_pairs"][a]["samples"]]
    assert gap, "the photograph pairs reach every arm the fields reach: nothing recorded to close"


if __name__ == "__main__":
    if "--write" in sys.argv:
        json.dump(derive(), open(GOLDEN, "w"), indent=1, sort_keys=True)
        print("wrote", GOLDEN)
    else:
        print(json.dumps(derive(), indent=1, sort_keys=True))
