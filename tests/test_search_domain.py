"""CPU: which arm of which value branch of phase A (the block search: gz_block_zeroing_orders[_masked]) the
parity tests' inputs take, counted by the oracle's search census (orc_branch_census' search_* arms: test
infrastructure, independent of the kernels).

The search cases of tests/fields.py, at the sizes the GPU suite runs them at, must take every arm on at least one
named case; the arms they do not take are listed with the reason and what was tried.  The counts are recorded in
tests/golden/search_census.json beside what the photograph cases of the GPU suite (case_block_search,
case_block_search420, case_block_search_masks444, the search of case_global_order) reach, and re-derived here.
(`python tests/test_search_domain.py --write` regenerates the file.)"""
import json
import os
import sys

import numpy as np

import fields
import images
import parity_cases as pc
from checkers import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "search_census.json")

GPU_SIZE = (93, 59)       # tests/test_gpu_parity.py: test_search_domain, test_compare_blocks_on_search_domain
GPU_SIZE_420 = (85, 53)   # test_search_domain_420: luma grid 11 x 7, chroma grid 6 x 4

# Arms no search case takes.  A case that does take one makes the test below fail as a stale entry.
UNREACHED = {
    "search_err_equals_limit":
        "an error is the float of a square root of a sum of FP64 products; the limit is the target as a float.  No "
        "block error of any case is bit-equal to its target (tried: the three targets 0.971769, 0.3, 3.0 and 50, 500 "
        "on all families, 17 000 to 18 000 distinct errors per noise case).  A target copied from a computed error "
        "would be a case made for the code under test, so `<=` against `<` at the cut stays unseen: errors that are "
        "exactly 0.0 do not help either, a target of 0 keeps nothing on any photograph",
}
# Not an arm of the oracle at all: std::sort is opaque to it.
NOT_COUNTED = {
    "rank_heap_sort_fallback":
        "k_rank_candidates restates libstdc++'s introsort; its heap-sort fall-back needs a list that defeats the "
        "median-of-three partition 2*floor(log2 n) times.  The oracle ranks with std::sort itself and cannot count it; "
        "no search case was built to drive it (the 189-element lists of the noise and uniform cases are random).  "
        "tests/cpp/test_rank_sort.cc drives the fall-back with crafted keys through gz_probe_rank_sort",
}


def _bees_cases():
    """The photograph inputs of phase A's existing GPU tests: (name, rgb, orig, cand, frame420, mask, lookahead,
    new_model), all at target 0.971769."""
    def crop(w, h, x0, y0):
        return images.crop(w, h, x0, y0) if max(w, h) <= 444 else images.tiled(w, h)

    def c444(w, h, x0, y0, qs):
        rgb = crop(w, h, x0, y0)
        h, w, _ = rgb.shape   # (a crop that reaches past the photograph is smaller than asked for)
        co = oracle.encode_rgb(rgb)
        return rgb, co, oracle.reconstruct(co, w, h, np.full((3, 64), qs, np.int32))[0]

    def c420(w, h, x0, y0, qs):
        rgb = crop(w, h, x0, y0)
        h, w, _ = rgb.shape
        orig = oracle.downsample(oracle.encode_rgb(rgb), w, h)
        return rgb, orig, oracle.reconstruct420(orig, w, h, np.full((3, 64), qs, np.int32))[0]

    for w, h, x0, y0, qs in ((45, 27, 300, 150, 3), (64, 40, 10, 10, 2), (444, 258, 0, 0, 2),   # case_block_search
                             (444, 258, 300, 150, 3), (61, 43, 300, 150, 3)):                    # case_global_order
        yield (f"block_search {w}x{h} q={qs}",) + c444(w, h, x0, y0, qs) + (False, 7, 3, True)
    for w, h, x0, y0, qs, la, nm in ((45, 27, 100, 60, 3, 3, True), (130, 75, 10, 10, 2, 3, True),
                                     (64, 48, 10, 10, 2, 2, False)):
        for mask in (1, 6):
            yield (f"block_search420 {w}x{h} mask {mask}",) + c420(w, h, x0, y0, qs) + (True, mask, la, nm)
    for w, h, x0, y0, la, nm in ((96, 64, 100, 60, 3, True), (61, 43, 50, 60, 1, True), (61, 43, 50, 60, 2, True),
                                 (61, 43, 50, 60, 5, False)):
        for mask in (7, 1, 6):
            yield (f"block_search_masks444 {w}x{h} lookahead {la} mask {mask}",) + c444(w, h, x0, y0, 3) + \
                (False, mask, la, nm)


def bees_census():
    out = {}
    for name, rgb, orig, cand, f420, mask, la, nm in _bees_cases():
        oc = oracle.comparator(rgb, 0.971769)
        oracle.census_reset()
        oc.block_zeroing_orders_masked(cand, orig, f420, mask, la, nm)
        out[name] = oracle.search_census()
        oc.close()
    return out


def search_cases_with_expected():
    """(case, offsets, indices, errors, census) of every search case at the GPU sizes."""
    for case in fields.search_cases(*GPU_SIZE):
        yield (case,) + pc.search_expected(case, *GPU_SIZE, False)
    for case in fields.search_cases_420(*GPU_SIZE_420):
        yield (case,) + pc.search_expected(case, *GPU_SIZE_420, True)


def _merged(per_case):
    arms = sorted(oracle.search_census())
    out = {}
    for a in arms:
        best = max(per_case, key=lambda n: per_case[n][a])
        out[a] = {"count": sum(c[a] for c in per_case.values()),
                  "most_on": best if per_case[best][a] else ""}
    return out


def derive():
    search = {case.name: census for case, _, _, _, census in search_cases_with_expected()}
    bees = bees_census()
    return {
        "arms": sorted(oracle.search_census()),
        "sizes": {"444": "%dx%d" % GPU_SIZE, "420": "%dx%d" % GPU_SIZE_420},
        "bees_cases": _merged(bees),
        "search_cases": _merged(search),
        "per_search_case": {n: {a: v for a, v in c.items() if v} for n, c in search.items()},
    }


_derived = None


def derived():
    global _derived
    if _derived is None:
        _derived = derive()
    return _derived


def test_search_cases_take_every_arm_or_it_is_listed():
    d = derived()
    assert set(UNREACHED) <= set(d["arms"]), "an arm listed as unreached does not exist"
    assert not set(NOT_COUNTED) & set(d["arms"])
    missed = [a for a in d["arms"] if d["search_cases"][a]["count"] == 0 and a not in UNREACHED]
    assert not missed, f"arms no search case takes: {missed}"
    stale = [a for a in UNREACHED if d["search_cases"][a]["count"] > 0]
    assert not stale, stale
    for a in d["arms"]:   # reached means: by a case with a name
        assert (d["search_cases"][a]["most_on"] != "") == (d["search_cases"][a]["count"] > 0)


def test_census_equals_the_recorded_one():
    """tests/golden/search_census.json is the record of the gap: per arm, what the photograph cases reach beside what
    the search cases reach."""
    rec = json.load(open(GOLDEN))
    assert derived() == rec
    gap = [a for a in rec["arms"] if rec["search_cases"][a]["count"] > 0 and rec["bees_cases"][a]["count"] == 0]
    assert gap, "the photograph cases reach every arm the search cases reach: nothing recorded to close"


def test_families_meet_their_conditions():
    """What each family is in the set for, so that a change to a generator that empties it fails here."""
    by = {case.name: (case, off, idx, err, census) for case, off, idx, err, census in search_cases_with_expected()}
    nb = ((GPU_SIZE[0] + 7) // 8) * ((GPU_SIZE[1] + 7) // 8)
    # zero_error: lists of errors that are exactly 0.0, ties at every step, every list kept whole
    _, off, _, err, cen = by["zero_error/white"]
    assert (err == 0.0).sum() >= 500, (err == 0.0).sum()
    assert cen["search_err_zero"] > 0 and cen["search_lookahead_tie_kept_first"] > 0
    assert cen["search_list_kept_whole"] == nb and cen["search_rank_equal_scores"] > 0
    for name in ("zero_error/black", "zero_error/grey"):
        assert (by[name][3] == 0.0).sum() >= 500 and by[name][4]["search_lookahead_tie_kept_first"] > 0, name
    # target: full lists of 189 candidates, every one cut at 0.3 (none to nothing), every one kept whole at 3.0
    lo, hi = by["target/noise/0.3"][4], by["target/noise/3.0"][4]
    assert lo["search_list_has_189"] >= 10 and hi["search_list_has_189"] >= 10
    assert lo["search_list_cut"] == nb and lo["search_list_cut_to_nothing"] == 0 and lo["search_list_kept_whole"] == 0
    assert hi["search_list_kept_whole"] == nb and hi["search_list_cut"] == 0
    assert np.diff(by["target/noise/3.0"][1]).max() == 189
    # saturating: both clamps of the search's IDCT and of its colour transform, by the million; lists cut to nothing
    for name in ("saturating/x4", "saturating/uniform2040/500.0", "saturating/extremes/500.0",
                 "saturating/sparse_wide/500.0"):
        cen = by[name][4]
        for arm in ("search_idct_pixel_clamped_low", "search_idct_pixel_clamped_high", "search_rgb_clamped_low",
                    "search_rgb_clamped_high"):
            assert cen[arm] >= 100000, (name, arm, cen[arm])
        assert np.isfinite(by[name][3]).all(), name
    assert by["saturating/x4"][4]["search_list_cut_to_nothing"] > 0
    assert by["saturating/uniform2040/500.0"][4]["search_list_has_189"] >= 10
    assert np.abs(by["saturating/extremes/500.0"][0].cand.astype(np.int32)).max() == 32768
    assert (by["saturating/extremes/500.0"][3] == 0.0).sum() >= 500
    # foreign_orig: the ranking of a foreign original differs from the ranking of the candidate's own source
    own = by["field/photo_zero_rect"]
    for name in ("foreign_orig/noise", "foreign_orig/extremes", "foreign_orig/extremes/old_model"):
        case, off, idx, err, _ = by[name]
        assert case.foreign and np.array_equal(case.cand, own[0].cand) and not np.array_equal(case.orig, own[0].orig)
        assert not (len(idx) == len(own[2]) and np.array_equal(idx, own[2])), name
    assert by["foreign_orig/extremes"][0].orig.min() == -32768
    # params: a look-ahead that is no multiple of the kernel's batch of three candidates
    assert by["params/noise/lookahead7"][0].lookahead % 3 and by["params/noise/lookahead1"][0].lookahead == 1
    # 4:2:0: the chroma search keeps candidates in most cells of the five colour fields at the wide target, and
    # in next to none of two of them at the encoder's
    cells = ((GPU_SIZE_420[0] + 15) // 16) * ((GPU_SIZE_420[1] + 15) // 16)
    assert cells == 24
    for name in fields.SEARCH_FIELDS_420:
        kept = np.diff(by[f"420/{name}/3.0/mask6"][1])
        assert kept.size == cells and (kept > 0).sum() >= 16, (name, (kept > 0).sum())
    assert (np.diff(by[f"420/primaries/{fields.TARGET}/mask6"][1]) > 0).sum() == 0
    assert (np.diff(by[f"420/noise/{fields.TARGET}/mask6"][1]) > 0).sum() <= 3
    assert (by["420/white/tiny_ac/mask1"][3] == 0.0).sum() >= 30
    # ... and sub-blocks of the chroma cells lie outside the image on both axes: the luma grid is odd in x and in y,
    # and the corner cell, with three of its four sub-blocks outside, has candidates
    assert ((GPU_SIZE_420[0] + 7) // 8) % 2 == 1 and ((GPU_SIZE_420[1] + 7) // 8) % 2 == 1
    cen = by["420/noise/3.0/mask6"][4]
    assert cen["search420_subblock_outside_right"] > 0 and cen["search420_subblock_outside_below"] > 0
    assert cen["search420_subblock_outside_image"] < cen["search420_subblock_outside_right"] + \
        cen["search420_subblock_outside_below"], "no sub-block outside on both axes at once"
    assert np.diff(by["420/noise/3.0/mask6"][1])[-1] > 0
    assert cen["search420_max_from_later_subblock"] > 0
    # the merged set
    m = derived()["search_cases"]
    assert m["search_lookahead_tie_kept_first"]["count"] > 0 and m["search420_subblock_outside_image"]["count"] > 0


def test_evaluations_follow_the_closed_form():
    """search_evaluations, the oracle's count of CompareBlock calls, against the closed form gz_search_evaluations
    uses, from the definition: step s of a block with n candidates compares min(lookahead, n - s) of them, on every
    sub-block of its cell that lies inside the image.  (The device's figure is compared with the oracle's count in
    case_search_domain.)"""
    for (w, h), gen, f420 in ((GPU_SIZE, fields.search_cases, False), (GPU_SIZE_420, fields.search_cases_420, True)):
        for case in gen(w, h):
            census = pc.search_expected(case, w, h, f420)[3]
            chroma = f420 and case.comp_mask == 6
            s = 16 if chroma else 8
            gw, gh = (w + s - 1) // s, (h + s - 1) // s
            cand = np.asarray(case.cand).reshape(-1, 64)
            nb = ((w + 7) // 8) * ((h + 7) // 8)
            first = [0, nb, nb + gw * gh] if f420 else [0, nb, 2 * nb]
            total = 0
            for b in range(gw * gh):
                n = sum(int((cand[first[c] + b, 1:] != 0).sum()) for c in range(3) if case.comp_mask >> c & 1)
                e = sum(min(case.lookahead, n - step) for step in range(n))
                sub = 1
                if chroma:
                    bx, by = b % gw, b // gw
                    sub = sum(8 * (2 * bx + ox) < w and 8 * (2 * by + oy) < h for ox in (0, 1) for oy in (0, 1))
                total += e * sub
            assert census["search_evaluations"] == total, case.name


if __name__ == "__main__":
    if "--write" in sys.argv:
        json.dump(derive(), open(GOLDEN, "w"), indent=1, sort_keys=True)
        print("wrote", GOLDEN)
    else:
        print(json.dumps(derive(), indent=1, sort_keys=True))
