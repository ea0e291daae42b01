"""The restatement that judges the heat map tests (tests/heatmap_cases.py: ScoreToRgb with math.pow, the fuzzy functions
with math.exp) pinned to the reference itself: butteraugli::CreateHeatMapImage, ButteraugliFuzzyClass and
ButteraugliFuzzyInverse out of oracle/_ref/libgz_ref.so, through the helper tests/cpp/heatmap_ref.cc, which this file
compiles into a temporary directory.  Every comparison is for equality, doubles with ==.  CPU only; skipped where
oracle/_ref is not built."""
import numpy as np
import pytest

import heatmap_cases as hc


@pytest.fixture(scope="module")
def reflib(tmp_path_factory):
    lib = hc.reference_helper(tmp_path_factory.mktemp("heatmap_ref"))
    if lib is None:
        pytest.skip("oracle/_ref/libgz_ref.so not built")
    return lib


def test_the_fuzzy_functions_are_the_references(reflib):
    for s in np.linspace(0, 4, 10000):
        assert hc.fuzzy_class(float(s)) == reflib.ref_fuzzy_class(float(s)), s
    rng = np.random.default_rng(7)
    for seek in [0.5, 1.0, 1.5] + list(rng.uniform(0.01, 1.99, 50)):
        assert hc.fuzzy_inverse(float(seek)) == reflib.ref_fuzzy_inverse(float(seek)), seek
    assert hc.default_thresholds() == (reflib.ref_fuzzy_inverse(1.5), reflib.ref_fuzzy_inverse(0.5))


@pytest.mark.parametrize("thresholds", [None, hc.OTHER_THRESHOLDS], ids=["default", "other"])
def test_the_restatement_is_the_reference_on_every_synthetic_plane(reflib, thresholds):
    good, bad = thresholds or hc.default_thresholds()
    hc.assert_the_cases_reach_what_they_claim(good, bad)
    for i, plane in enumerate(hc.synthetic_planes(good, bad)):
        assert np.array_equal(hc.expected_heat(plane, good, bad), hc.reference_heat(reflib, plane, good, bad)), i
    for w, h in hc.SIZES:
        plane = hc.plane_of_size(w, h, good, bad, seed=100 * h + w)
        assert np.array_equal(hc.expected_heat(plane, good, bad), hc.reference_heat(reflib, plane, good, bad)), (w, h)


def test_the_golden_fixture_is_the_references_output(reflib):
    good, bad = hc.default_thresholds()
    plane, heat = hc.golden()
    assert np.array_equal(plane.view(np.uint32), hc.golden_plane(good, bad).view(np.uint32))
    assert np.array_equal(hc.reference_heat(reflib, plane, good, bad), heat)
    assert len(np.unique(heat.reshape(-1, 3), axis=0)) > 100
