"""CPU: phase B's domain (tests/order_domain.py).

1. The restatements are pinned before they judge a kernel: the weights equal the oracle's block_weights(_factor) -- and
   the reference's where oracle/_ref is built -- on distance maps that realise every family's block maxima, and the host
   form gz_block_weights(_factor) through gz_probe_set_block_max; Quantize equals the oracle's on every int16 at eight
   quantisers; the construction loop, the advance, the steps and the statistics change equal the loops of
   case_global_order / case_global_order420 on their photograph inputs (asserted inside those cases).
2. Which arm each input takes, counted by the restatements: every arm is taken by a named family or is listed in
   UNREACHED with the reason.  The counts are recorded in tests/golden/order_census.json beside what the photograph cases
   reach (`python tests/test_order_domain.py --write` regenerates the file).
3. What each family is in the set for.
4. Every family through the emulation build of the kernels.
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
if ROOT not in sys.path:
    sys.path.insert(1, ROOT)     # (run as a script: --write)
import build_emu  # noqa: E402
import order_domain as od  # noqa: E402
import parity_cases as pc  # noqa: E402
from checkers import assert_bits_equal, oracle, ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "order_census.json")

# Arms no family takes.  A family that does take one makes the census test fail as a stale entry.
UNREACHED = {
    "last/float_product_differs":
        "min_coeffs_to_change is a FLOAT product, truncated; for per_block 2.0, 0.2f and 0.8f and every blocks_to_change "
        "up to 16 900 it truncates to the integer the exact product truncates to (all of them tried: "
        "test_families_meet_their_conditions), so no input of the domain tells the two apart",
}

# What runs on the device only, and why.
DEVICE_ONLY = {
    "descent, 1040 x 1040, every value":
        "the emulation runs the workgroups of the twelve levels one after the other over 338 000 entries: some 13 000 "
        "descents there take hours.  It runs every 997th value of the large context; tests/test_order_gpu.py runs all",
}

# The photograph cases of the existing tests whose arms are recorded beside the families'.  (444 x 258, the other size
# of test_gpu_parity.test_global_order, takes 50 s under the emulation -- phase A and a Compare -- and is left out: with
# 1848 blocks it stays in one trip over the group sums and at per = 1, like 61 x 43.)
PHOTO = (("global_order 61x43", lambda L, cen: pc.case_global_order(L, 61, 43, x0=0, y0=0, census=cen)),
         ("global_order420 130x75", lambda L, cen: pc.case_global_order420(L, 130, 75, oracle, x0=100, y0=60, census=cen)))

WEIGHT_PARAMS = [(f, gi, t) for f in od.WEIGHT_FAMILIES for gi in range(len(od.WEIGHT_GRIDS)) for t in od.TARGETS]
DESCENT_PARAMS = [(p, short) for p in od.PER_BLOCK for short in (False, True)]


@pytest.fixture(scope="module")
def L():
    return emu()


_emu = None


def emu():
    global _emu
    if _emu is None:
        from guetzli_amd.capi import Library
        _emu = Library(build_emu.build())
    return _emu


def _all_modes():
    return [(d, r, m) for d in (1, -1) for r in od.RADII for m in od.MULS]


def family_census():
    out = {}
    for family, gi, target in WEIGHT_PARAMS:
        g = od.WEIGHT_GRIDS[gi]
        cen = out.setdefault(f"weights {family} {g.name} target {target}", {})
        for case in od.weight_cases(family, g, target):
            for d, r, m in _all_modes():
                case.reference(d, r, m, cen)
    for family in od.ORDER_FAMILIES:
        cen = out.setdefault(f"order {family}", {})
        for case in od.order_cases(family):
            case.reference(cen)
    for family in od.STEP_FAMILIES:
        cen = out.setdefault(f"steps {family}", {})
        for case in od.step_cases(family):
            case.reference(cen)
    for big in (False, True):
        g = od.Grid(*od.BIG) if big else od.grid_of_blocks(17, 13)
        for p, short in DESCENT_PARAMS:
            cen = out.setdefault(f"descent per_block {p} {'short' if short else 'long'} {g.gn} blocks", {})
            for btc in od.btc_values(p, g.gn):
                n = btc * (1 if short else od.DESCENT_CNT)
                if n > 16 and (not big or btc > 221):
                    od.derived_last(p, btc, n, cen)
    return out


def photo_census():
    out = {}
    for name, run in PHOTO:
        cen = out.setdefault(name, {})
        run(emu(), cen)          # (asserts the restatements against the cases' own loops on the way)
    return out


def _merged(per_case, arms):
    out = {}
    for a in arms:
        best = max(per_case, key=lambda n: per_case[n].get(a, 0))
        total = sum(c.get(a, 0) for c in per_case.values())
        out[a] = {"count": total, "most_on": best if total else ""}
    return out


def derive():
    fam, photo = family_census(), photo_census()
    arms = sorted(set().union(*(c.keys() for c in fam.values()), *(c.keys() for c in photo.values())))
    rec = {"arms": arms, "photo_cases": _merged(photo, arms), "families": _merged(fam, arms),
           "device_only": DEVICE_ONLY, "unreached": UNREACHED}
    return rec, fam


_derived = None


def derived():
    global _derived
    if _derived is None:
        _derived = derive()
    return _derived


# ------------------------------------------------------------------------- the pins --
@pytest.mark.parametrize("gi", range(len(od.WEIGHT_GRIDS)))
def test_weights_equal_the_oracle(gi):
    """On distance maps whose block maxima are the families': block_weights / block_weights_factor of the oracle, and of
    the reference where it is built."""
    g = od.WEIGHT_GRIDS[gi]
    rgb = np.zeros((g.h, g.w, 3), np.uint8)
    n = 0
    for target in od.TARGETS:
        checkers = [oracle.comparator(rgb, target)] + ([ref.comparator(rgb, target)] if ref is not None else [])
        for family in od.WEIGHT_FAMILIES:
            for case in od.weight_cases(family, g, target):
                dm = od.distmap_of(case.bmax8, g) if case.use_distmap else np.zeros((g.h, g.w), np.float32)
                for d, r, m in _all_modes():
                    exp = case.reference(d, r, m)
                    for oc in checkers:
                        got = oc.block_weights_factor(d, r, m, 2, dm) if g.factor == 2 else oc.block_weights(d, r, m, dm)
                        assert_bits_equal(got, exp, f"{oc.chk.name}: {family} {g.name} {target} {d} {r} {m}")
                        n += 1
        for oc in checkers:
            oc.close()
    assert n >= 2 * len(od.WEIGHT_FAMILIES) * 16


def test_quantize_equals_the_oracle():
    """Every int16 at eight quantisers.  Where raw + delta leaves int16 (q = 32767 and |raw| beyond 16384: delta itself
    is narrowed to int16 first) the oracle wraps as the restatement and the kernel's casts do: kept."""
    raw = np.arange(-32768, 32768, dtype=np.int64)
    wrapped = 0
    for q in (1, 2, 3, 5, 9, 255, 256, 32767):
        exp = np.concatenate([oracle.quantize_block(raw[i:i + 64].astype(np.int16), np.full(64, q, np.int32))[0]
                              for i in range(0, 65536, 64)])
        assert_bits_equal(od.quantize(raw, q), exp, f"Quantize, q = {q}")
        r = np.fmod(raw, q)
        exact = raw + np.where(2 * r > q, q - r, np.where(-2 * r > q, -q - r, -r))
        wrapped += int((np.abs(exact) > 32767).sum())
    assert wrapped > 0


def test_photograph_cases_agree_with_the_restatements():
    """case_global_order / case_global_order420 assert order_domain's weights, construction loop, advance, steps and
    statistics change against their own loops and the oracle; they ran to the end."""
    photo = derived()[0]["photo_cases"]
    assert photo["fill/n/1to16"]["count"] > 0 and photo["steps/precious/other_k"]["count"] > 0


def test_families_realise_their_maxima_as_maps():
    g = od.WEIGHT_GRIDS[3]
    case = od.weight_cases("random", g, od.TARGETS[0])[0]
    dm = od.distmap_of(case.bmax8, g)
    got = dm.reshape(g.bh, 8, g.bw, 8).max(axis=(1, 3)).reshape(-1)
    assert_bits_equal(got, case.bmax8, "block maxima of the map")
    assert (dm > 0).sum() <= g.nb


# ----------------------------------------------------------------------- the census --
def test_families_take_every_arm_or_it_is_listed():
    rec = derived()[0]
    assert set(UNREACHED) <= set(rec["arms"]), "an arm listed as unreached does not exist"
    missed = [a for a in rec["arms"] if rec["families"][a]["count"] == 0 and a not in UNREACHED]
    assert not missed, f"arms no family takes: {missed}"
    stale = [a for a in UNREACHED if rec["families"][a]["count"] > 0]
    assert not stale, stale
    for a in rec["arms"]:   # reached means: by a case with a name
        assert (rec["families"][a]["most_on"] != "") == (rec["families"][a]["count"] > 0)


def test_census_equals_the_recorded_one():
    """tests/golden/order_census.json is the record of the gap: per arm, what the photograph cases reach beside what
    the families reach."""
    stored = json.load(open(GOLDEN))
    assert derived()[0] == stored
    gap = [a for a in stored["arms"] if stored["families"][a]["count"] > 0 and stored["photo_cases"][a]["count"] == 0]
    for a in ("w/own/gt", "w/own/gt_hug", "w/local/le_hug", "w/mix/gt", "w/mix/gt_hug", "w/tdf_above_td", "w/tdf_below_td",
              "w/cheb/0/full", "w/cheb/3/clipped", "w/radius_covers_grid", "fill/clamp", "fill/group_trips/2",
              "fill/group/empty_before_live", "fill/below/eq", "steps/per/2", "steps/per/3plus", "quantize/tie_2r_eq_q",
              "last/capped", "last/multiple_of_10"):       # (no block of the photograph cases is hot at all)
        assert a in gap, a


def test_families_meet_their_conditions():
    """What each family is in the set for, so that a change to a generator that empties it fails here."""
    fam = derived()[1]

    def cen(name):
        return fam[name]
    big_grids = [g for g in od.WEIGHT_GRIDS if g.gn >= 63]
    for target, side in zip(od.TARGETS, ("w/tdf_above_td", "w/tdf_below_td")):
        for g in od.WEIGHT_GRIDS:
            c = cen(f"weights hug/own {g.name} target {target}")
            # float(td) on its side of td under 0.97, equal to it under 1.0
            assert c[side] > 0 and c["w/tdf_equals_td"] > 0 and c.get("w/tdf_below_td" if side.endswith("above_td") else "w/tdf_above_td", 0) == 0
            assert c["w/own/le_hug"] > 0 and c["w/own/gt_hug"] > 0, (g.name, target)
            c = cen(f"weights hug/local {g.name} target {target}")
            assert c["w/local/le_hug"] > 0 and c["w/local/gt_hug"] > 0, (g.name, target)
            if g.gn > 1:
                c = cen(f"weights hug/mix {g.name} target {target}")
                assert c["w/mix/le_hug"] > 0 and c["w/mix/gt_hug"] > 0, (g.name, target)
        for g in big_grids:
            c = cen(f"weights lone {g.name} target {target}")
            assert all(c[f"w/cheb/{d}/clipped"] > 0 for d in range(5)), g.name
            if min(g.gw, g.gh) > 8:
                assert all(c[f"w/cheb/{d}/full"] > 0 for d in range(5)), g.name
    # a radius larger than the grid; 1 x N and N x 1; the ragged 16 x 16 grouping
    for name, arm in (("444/7 8x8", "grid"), ("420/6 24x24", "grid"), ("444/7 72x8", "one_axis"), ("444/7 8x72", "one_axis")):
        assert cen(f"weights lone {name} target {od.TARGETS[0]}")[f"w/radius_covers_{arm}"] > 0
    for name in ("420/6 136x104", "420/6 24x24"):
        assert cen(f"weights random {name} target {od.TARGETS[0]}")["w/group/ragged"] > 0
    g = od.WEIGHT_GRIDS[3]
    for target in od.TARGETS:
        for case in od.weight_cases("all_cold", g, target):
            assert not any(case.reference(-1, r, m).any() for r in od.RADII for m in od.MULS)
        for case in od.weight_cases("all_hot", g, target):
            assert not any(case.reference(1, r, m).any() for r in od.RADII for m in od.MULS)
        for case in od.weight_cases("nodistmap", g, target):
            assert case.reference(1, 1, 1.0).all() and not case.reference(-1, 4, 0.97).any()
        for case in od.weight_cases("pair", g, target):          # where two neighbourhoods overlap the nearer block wins
            w = case.reference(-1, 4, 1.0).reshape(g.gh, g.gw)
            assert len(set(np.round(1 / w[w > 0]).astype(int).tolist())) >= 4
    # the construction families
    c = cen("order fill/edges")
    assert all(c[f"fill/n/eq{k}"] >= 20 for k in (16, 17, 32, 33)) and c["fill/n/0"] > 0 and c["fill/n/gt32"] > 0
    for case in od.order_cases("fill/edges"):
        nb = case.reference()[0]
        per_block = np.bincount(nb, minlength=case.g.gn)
        assert set(per_block.tolist()) <= set(od.FILL_EDGES)
    assert sum(set(np.bincount(c.reference()[0], minlength=c.g.gn).tolist()) == set(od.FILL_EDGES)
               for c in od.order_cases("fill/edges")) >= 2       # from both directions
    assert cen("order fill/overrun")["fill/clamp"] > 50
    c = cen("order groups")
    assert c["fill/group_trips/2"] == 5 and c["fill/group/empty_before_live"] > 10 and c["fill/group/full_last"] > 0
    assert {case.g.gn for case in od.order_cases("groups")} == {255, 256, 257, 1023, 16900}
    alt = [case for case in od.order_cases("groups") if case.direction > 0 and (case.bmax8[1::2] > 0).all() and not case.bmax8[::2].any()]
    assert len(alt) == 5 and all((case.weights()[::2] == 1).all() and not case.weights()[1::2].any() for case in alt)
    c = cen("order ties")
    assert c["fill/below/eq"] > 100 and c["fill/below/lt"] > 100 and c["fill/below/gt"] > 100
    for case in od.order_cases("ties"):
        assert len(set(case.err.tolist())) == 4
    c = cen("order signs")
    assert c["fill/val/negative"] > 100 and c["fill/val/zero"] > 100
    c = cen("order small")
    assert c["fill/val/denormal_operands"] > 1000
    ws = set(od.order_cases("small")[0].weights().tolist())
    assert np.float32(1) / np.float32(3) in ws and np.float32(1) / np.float32(5) in ws
    # the steps
    c = cen("steps precious/edges")
    assert all(c[f"steps/precious/limit{L}/{yn}"] >= 16 for L in (4, 8) for yn in ("yes", "no")) and c["steps/precious/newval_nonzero"] > 0
    for case in od.step_cases("precious/edges"):
        hf = {od.sum_of_hf(b) for b in case.orig[:64]}
        assert hf == {59, 60} and np.abs(case.orig[:64].astype(int)).max() == 2000
        assert {abs(int(b[k])) for b in case.orig[:64] for k in (1,)} >= {3, 4, 7, 8}
    c = cen("steps quantize/ties")
    assert min(c["quantize/tie_2r_eq_q"], c["quantize/tie_neg_2r_eq_q"], c["quantize/round_up"], c["quantize/round_down_negative"],
               c["quantize/q_gt_abs_raw"], c["quantize/q_is_1"]) > 500
    assert sorted(set(od.step_cases("counts")[0].calls[0][3].tolist())) == [1, 63, 64, 65, 189]
    c = cen("steps n/tails")
    assert c["steps/per/1"] == 6 and c["steps/per/2"] == 1 and c["steps/per/3plus"] == 1 and c["steps/wavefront/not_live"] > 0
    assert sorted(len(call[2]) for case in od.step_cases("n/tails") for call in case.calls) == [1, 3, 4, 5, 8191, 8192, 8193, 16900]
    c = cen("steps runs")
    assert min(c["steps/zrl/more"], c["steps/zrl/fewer"], c["steps/eob/more"], c["steps/eob/fewer"]) > 0
    case = od.step_cases("runs")[0]
    deltas = [d for _, d in case.reference()]
    assert deltas[0][0, 0xf0] < 0 and deltas[1][0, 0xf0] == -deltas[0][0, 0xf0] and deltas[0][0, 0] > 0     # ZRLs go and come back
    assert (case.reference()[0][0] == 0).all() and (case.reference()[1][0][:, 63] != 0).any()
    assert not od.step_cases("plain")[0].with_statistics
    assert [c.g.mask for c in od.step_cases("420")] == [1, 6]
    # the descent's position
    for p in od.PER_BLOCK:
        c = cen(f"descent per_block {p} long 221 blocks")
        assert min(c["last/uncapped"], c["last/zero"], c["last/multiple_of_10"], c["last/rounded_down"]) > 0
        assert set(range(61)) <= set(od.btc_values(p, 221))
    assert cen("descent per_block 2.0 short 221 blocks")["last/capped"] > 10
    assert cen("descent per_block 2.0 short 16900 blocks")["last/capped"] > 100
    for p in od.PER_BLOCK:       # (UNREACHED: the float product never truncates to another integer than the exact one)
        b = np.arange(16901)
        assert ((np.float32(p) * b.astype(np.float32)).astype(np.int64) == (np.float64(np.float32(p)) * b).astype(np.int64)).all()


# --------------------------------------------------------------- the emulation build --
@pytest.fixture(scope="module")
def contexts(L):
    cache = pc.TargetContexts(L)
    yield cache
    cache.close()


@pytest.mark.parametrize("family,gi,target", WEIGHT_PARAMS)
def test_emulation_weights(contexts, family, gi, target):
    """... and gz_block_weights(_factor), the host form, on the maxima the hook installed."""
    pc.case_order_weights(contexts, family, gi, target, host_form=True)


@pytest.mark.parametrize("family", od.ORDER_FAMILIES)
def test_emulation_order(contexts, family):
    pc.case_order_build(contexts, family)


@pytest.mark.parametrize("family", od.ADVANCE_FAMILIES)
def test_emulation_advance(contexts, family):
    pc.case_order_advance(contexts, family)


@pytest.mark.parametrize("family", od.STEP_FAMILIES)
def test_emulation_steps(L, contexts, family):
    pc.case_order_steps(L, contexts, family)


@pytest.mark.parametrize("per_block,short", DESCENT_PARAMS)
def test_emulation_descent(contexts, per_block, short):
    pc.case_order_descent(contexts, per_block, big=False, short=short)
    pc.case_order_descent(contexts, per_block, big=True, short=short, every=997)     # (DEVICE_ONLY)


def test_hooks_reject_what_they_cannot_install(L):
    g = od.grid_of_blocks(3, 2)
    with L.context(np.zeros((g.h, g.w, 3), np.uint8), 1.0) as ctx:
        off = np.arange(g.gn + 1, dtype=np.int32)
        bad = off.copy()
        bad[-1] = bad[-2] + 193                        # more than 192 candidates in a block
        z8, zf = np.zeros(400, np.uint8), np.zeros(400, np.float32)
        assert L.lib.gz_probe_set_search(ctx.handle, 7, bad.ctypes.data, z8.ctypes.data, zf.ctypes.data) == -1
        bad = off[::-1].copy()
        assert L.lib.gz_probe_set_search(ctx.handle, 7, bad.ctypes.data, z8.ctypes.data, zf.ctypes.data) == -1
        assert L.lib.gz_probe_set_search(ctx.handle, 8, off.ctypes.data, z8.ctypes.data, zf.ctypes.data) == -1
        assert L.lib.gz_probe_order_state(ctx.handle, zf.ctypes.data, None) == -4      # no search, no order yet
        ctx.probe_set_search(off, z8[:g.gn], zf[:g.gn])
        assert L.lib.gz_probe_order_state(ctx.handle, zf.ctypes.data, None) == -4      # no order yet
        ctx.order_build_auto_begin(1, 1, 1.0, False, np.zeros(g.gn, np.int32))
        ctx.probe_set_search(off, z8[:g.gn], zf[:g.gn])                                 # voids the pending order
        assert L.lib.gz_order_build_auto_end(ctx.handle, zf.ctypes.data, zf.ctypes.data, zf.ctypes.data) == -4
        ctx.set_frame(2)
        assert L.lib.gz_probe_set_search(ctx.handle, 7, off.ctypes.data, z8.ctypes.data, zf.ctypes.data) == -1


if __name__ == "__main__":
    rec = derive()[0]
    if "--write" in sys.argv:
        json.dump(rec, open(GOLDEN, "w"), indent=1, sort_keys=True)
        print("wrote", GOLDEN)
    else:
        print(json.dumps(rec, indent=1, sort_keys=True))
