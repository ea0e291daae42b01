"""CPU: the device scan coder's domain (tests/entropy_domain.py).

1. The reference coder is pinned: on the codes the product builds (jpeg_head) its head + stuffed bytes + EOI equal the
   host writer's file -- and the reference's own WriteJpeg where oracle/_ref is built -- for every family at every
   shape of the GPU tests and for the photograph inputs of case_jpeg_entropy / case_jpeg_entropy420.  Only then does it
   judge the kernels under code tables no writer produces.
2. Which arm each input takes, counted by the reference coder: every arm is taken by a named family under some kind of
   table at the GPU shapes, or is listed in UNREACHED with the reason.  The counts are recorded in
   tests/golden/entropy_census.json beside what the photograph cases reach (`python tests/test_entropy_domain.py
   --write` regenerates the file).
3. What each family is in the set for.
4. All families through the emulation build of the kernels (the GPU tests' shapes where the emulation can afford them).
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
import entropy_domain as ed  # noqa: E402
import parity_cases as pc  # noqa: E402
from checkers import oracle, ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "entropy_census.json")

# Arms no family takes at the GPU shapes.  A family that does take one makes the census test fail as a stale entry.
UNREACHED = {
    "mcu_span/444/gt8192":
        "with code lengths of at most 16 a 4:4:4 MCU is at most 3 * (63 * (16 + 15) + 16 + 16) = 5955 bits, 31 more "
        "for its start phase: below the 8192 bits k_jpeg_emit<3> stages.  Its unstaged path needs code lengths above "
        "16, which are outside the domain (tried: `dense` and `wide` under flat16, the longest MCUs the domain has)",
    "mcu_span/gray/gt8192":
        "a single-component MCU is one block, at most 63 * (16 + 15) + 16 + 16 = 1985 bits: the same argument for "
        "k_jpeg_emit<1>",
    "tiles/gt64":
        "a scan of more than 64 prefix-scan tiles has more than 131 072 MCUs (a 4:4:4 frame of 8.4 MPix); the shapes "
        "here stop at 4160.  k_scan_offsets' second look-back round is driven by gz_probe_scan_offsets instead "
        "(65 * 2048 + 1 values), the whole encodes of the large golden hashes run it inside a scan",
    "tiles/gt128":
        "as tiles/gt64: gz_probe_scan_offsets with 130 * 2048 + 77 values, a third look-back round",
}

PHOTO_444 = [(444, 258), (61, 43), (32, 32), (129, 9), (8, 8)]      # test_gpu_parity.test_jpeg_entropy
PHOTO_420 = [(444, 258), (61, 43), (32, 32), (129, 9)]              # test_gpu_parity.test_jpeg_entropy420


@pytest.fixture(scope="module")
def L():
    from guetzli_amd.capi import Library
    return Library(build_emu.build())


_host = None


def host_emu():
    global _host
    if _host is None:
        from guetzli_amd.encoder import HostLibrary
        _host = HostLibrary(build_emu.build_host())
    return _host


def _blocks_of(geom, coeffs):
    co = np.asarray(coeffs).reshape(-1, 64)
    n = [geom.nb, geom.nbc, geom.nbc] if geom.layout == "420" else [geom.nb] * 3
    first = np.concatenate([[0], np.cumsum(n)])
    return [co[first[c]:first[c + 1]] for c in range(geom.ncomp)]


def _pin(H, geom, coeffs, q, blocks, refs, failures, what, array_factor=None):
    """Reference coder under the product's codes == the host writer (== the reference's writer); returns the coding."""
    qq = np.ones((3, 64), np.int32) if q is None else q
    s = ed.symbolize(geom, blocks, qq)
    factor = geom.factor if array_factor is None else array_factor
    head, depth, code = H.jpeg_head(s.hist, geom.w, geom.h, q, geom.ncomp, factor)
    r = ed.encode(s, depth, code)
    got = head + r.stuffed + b"\xff\xd9"
    if got != H.write_jpeg(coeffs, geom.w, geom.h, q, factor=factor):
        failures.append(what + ": host writer")
    for name, f in refs:
        if got != f():
            failures.append(what + ": " + name)
    return s, r


def photo_census(failures):
    H = host_emu()
    out = {}
    for w, h in PHOTO_444:
        _, co, cases, wild = pc.jpeg_entropy_inputs(w, h)
        for i, (cq, q, is_grey) in enumerate(cases):
            geom = ed.Geom("gray" if is_grey else "444", w, h)
            refs = []
            if ref is not None and q is not None and not is_grey and cq is not wild:
                refs = [("reference WriteJpeg", lambda: ref.write_jpeg(co, w, h, q))]
            name = f"jpeg_entropy {w}x{h} case {i}"
            out[name] = _pin(H, geom, cq, q, _blocks_of(geom, cq), refs, failures, name)[1].census
    for w, h in PHOTO_420:
        import images
        orig = oracle.downsample(oracle.encode_rgb(images.crop(w, h, 0, 0)), w, h)
        for i, q in enumerate(pc.jpeg_entropy420_quants(w, h)):
            cq = oracle.reconstruct420(orig, w, h, q)[0]
            g420 = ed.Geom("420", w, h)
            chroma = np.asarray(cq).reshape(-1, 64)[g420.nb:]
            geom = g420 if chroma.any() else ed.Geom("gray", w, h)      # luma alone: one block per MCU, no padding
            refs = [("reference WriteJpeg (4:2:0)", lambda: ref.write_jpeg420(orig, w, h, q))] if ref is not None else []
            name = f"jpeg_entropy420 {w}x{h} q {i}"
            out[name] = _pin(H, geom, cq, q, _blocks_of(g420, cq)[:geom.ncomp], refs, failures, name, array_factor=2)[1].census
    return out


def family_census(failures, conditions):
    H = host_emu()
    out = {}
    for family in ed.FAMILIES:
        for layout, w, h in ed.SHAPES:
            case = ed.case(family, layout, w, h)
            geom = case.geom
            refs = []
            # (the reference's OutputImage quantises by rounding: it holds the same frame only where the coefficients
            # are multiples of q; its harness has room for 3 bytes per pixel)
            if ref is not None and case.multiples_of_q and layout != "gray":
                f = ref.write_jpeg420 if layout == "420" else ref.write_jpeg

                def write(f=f):
                    try:
                        return f(case.coeffs, w, h, case.q)
                    except AssertionError:
                        return None
                got_ref = write()
                if got_ref is not None:
                    refs = [("reference WriteJpeg", lambda: got_ref)]
            what = f"{family} {layout} {w}x{h}"
            s, r = _pin(H, geom, case.coeffs, case.q, case.blocks, refs, failures, what)
            coded = {"optimal": r}
            for kind in ("flat16", "skewed"):
                coded[kind] = ed.encode(s, *ed.tables(kind, s.hist))
            for kind, r in coded.items():
                out[f"{family} {kind} {layout} {w}x{h}"] = r.census
                conditions[(family, kind, layout, w, h)] = {
                    "pad": r.pad, "span_max": int(r.span.max()), "total_bits": r.total_bits,
                    "stuffed": r.stuffed_count, "multiples_of_q": case.multiples_of_q, "hist": s.hist}
    return out


def _merged(per_case, arms, label):
    out = {}
    for a in arms:
        best = max(per_case, key=lambda n: per_case[n][a])
        out[a] = {"count": sum(c[a] for c in per_case.values()), "most_on": label(best) if per_case[best][a] else ""}
    return out


def derive():
    failures, conditions = [], {}
    fam = family_census(failures, conditions)
    photo = photo_census(failures)
    arms = sorted(next(iter(fam.values())))
    rec = {
        "arms": arms,
        "shapes": ["%s %dx%d" % s for s in ed.SHAPES],
        "photo_cases": _merged(photo, arms, lambda n: n),
        "families": _merged(fam, arms, lambda n: n),
    }
    return rec, fam, failures, conditions


_derived = None


def derived():
    global _derived
    if _derived is None:
        _derived = derive()
    return _derived


def test_reference_coder_equals_the_writers():
    """Under the product's own codes: the reference coder's file == the host writer's == the reference's, on every
    family at every GPU shape and on the photograph inputs."""
    _, fam, failures, _ = derived()
    assert len(fam) == len(ed.FAMILIES) * len(ed.SHAPES) * len(ed.KINDS)
    assert not failures, failures[:10]


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
    """tests/golden/entropy_census.json is the record of the gap: per arm, what the photograph cases of the existing
    entropy tests reach beside what the families reach."""
    stored = json.load(open(GOLDEN))
    assert derived()[0] == stored
    gap = [a for a in stored["arms"] if stored["families"][a]["count"] > 0 and stored["photo_cases"][a]["count"] == 0]
    assert gap, "the photograph cases reach every arm the families reach: nothing recorded to close"
    for a in ("mcu_span/420/gt8192", "mcu_span/420/within64_above", "pad_block/corner", "run_exact/62", "dc_size/13to15/pos"):
        assert a in gap, a


def test_families_meet_their_conditions():
    """What each family is in the set for, so that a change to a generator that empties it fails here."""
    _, fam, _, cond = derived()

    def cen(family, kind, layout, w, h):
        return fam[f"{family} {kind} {layout} {w}x{h}"]
    # dense under 16-bit codes at 4:2:0: MCUs on both sides of the staging limit, and within 64 bits of it on each
    c = cen("dense", "flat16", "420", 448, 296)
    assert c["mcu_span/420/gt8192"] >= 100 and c["mcu_span/420/le8192"] >= 100
    assert c["mcu_span/420/within64_below"] >= 10 and c["mcu_span/420/within64_above"] >= 10
    assert cen("dense", "flat16", "420", 85, 53)["mcu_span/420/gt8192"] > 0
    assert cen("dense", "flat16", "420", 8, 8)["mcu_span/420/le8192"] == 1      # (three of its six blocks are padding)
    for layout, w, h in ed.SHAPES:
        g = ed.Geom(layout, w, h)
        real = sum(gw * gh for gw, gh in g.grid)
        c = cen("dense", "flat16", layout, w, h)   # no zero anywhere: no end-of-block but in the padding blocks
        assert c["eob/absent"] == real and c["eob/alone"] == g.nmcu * g.upm - real and c["eob/other"] == 0
        # pad/k ends with k bits of padding
        for k in range(8):
            assert cond[(f"pad/{k}", "flat16", layout, w, h)]["pad"] == k, (k, layout, w, h)
    # ff/ones: a stuffed byte at every position of a word and as the scan's last byte, under every kind of table
    for kind in ed.KINDS:
        for layout, w, h in (("444", 93, 59), ("420", 85, 53), ("gray", 93, 59), ("444", 24, 8)):
            c = cen("ff/ones", kind, layout, w, h)
            assert all(c[f"ff_at_byte/{j}"] > 0 for j in range(4)) and c["ff_last_byte"] == 1, (kind, layout, w, h)
    # ff/code: no extra bit is set, so every 0xFF is made of code bits alone; the skewed codes produce them
    c = cen("ff/code", "skewed", "444", 93, 59)
    assert c["ff_from_code_bits"] > 0 and c["ff_from_code_bits"] == sum(c[f"ff_at_byte/{j}"] for j in range(4))
    assert cen("ff/code", "skewed", "420", 85, 53)["ff_from_code_bits"] > 0
    # wide: sizes 12..14 of AC values, 13..15 of DC differences
    for layout, w, h in (("444", 93, 59), ("420", 85, 53)):
        c = cen("wide", "flat16", layout, w, h)
        assert c["ac_size/12to14"] > 0 and c["dc_size/13to15/pos"] > 0 and c["dc_size/13to15/neg"] > 0
        assert cond[("wide", "flat16", layout, w, h)]["hist"][0, :, 15].sum() > 0      # 16 + 15 = 31 bits in one unit
    # sparse under the product's codes: MCUs of a few bits, inside one word that both neighbours share
    assert cen("sparse", "optimal", "444", 93, 59)["mcu_in_one_word_shared_with_both_neighbours"] > 50
    assert cen("phase/tiny", "optimal", "gray", 93, 59)["mcu_in_one_word_shared_with_both_neighbours"] > 50
    c = cen("phase/walk", "flat16", "444", 93, 59)
    assert sum(c[f"mcu_phase/{p}"] > 0 for p in range(32)) >= 16
    # the symbol families: every (run, size) symbol of both tables, on the 4:2:0 frame too
    for layout in ("444", "420"):
        a, b = cen("symbols/cyclic", "flat16", layout, 448, 296), cen("symbols/single", "flat16", layout, 448, 296)
        for cls in ("luma", "chroma"):
            for r in range(16):
                for n in range(1, 12):
                    assert a[f"ac_sym/{cls}/{r:x}{n:x}"] > 0 and b[f"ac_sym/{cls}/{r:x}{n:x}"] > 0, (layout, cls, r, n)
    for layout, w, h in (("444", 93, 59), ("420", 85, 53)):
        c = cen("runs/exact", "flat16", layout, w, h)
        assert all(c[f"run_exact/{r}"] > 0 for r in ed.RUNS) and all(c[f"zrl_per_coeff/{z}"] > 0 for z in (1, 2, 3))
        assert all(c[f"eob/{e}"] > 0 for e in ("alone", "after_62", "absent", "other"))
        c = cen("dc/ladder", "flat16", layout, w, h)
        assert c["dc_size/0/zero"] > 0 and all(c[f"dc_size/{n}/{s}"] > 0 for n in range(1, 13) for s in ("pos", "neg"))
        c = cen("dc/extremes", "flat16", layout, w, h)
        assert c["dc_size/12/pos"] > 10 and c["dc_size/12/neg"] > 10
    # the quantiser families
    h = cond[("quant/huge", "flat16", "444", 93, 59)]["hist"]
    assert h.sum() == h[0, :, 0].sum() + h[1, :, 0].sum() == 2 * 3 * 96
    assert not cond[("quant/remainders", "flat16", "444", 93, 59)]["multiples_of_q"]
    case = ed.case("quant/remainders", "444", 93, 59)
    co = case.blocks[0].astype(np.int64)
    assert ((co < 0) & (co % case.q[0][None, :] != 0)).sum() > 100
    assert ed.case("quant/255", "444", 93, 59).blocks[0].min() == -32768
    # 4:2:0 geometry: the luma grid of 85 x 53 is odd on both axes -- padding to the right, below and in the corner,
    # and blocks predicted across them; an image of one luma block has one of each
    c = cen("dc/ladder", "flat16", "420", 85, 53)
    assert c["pad_block/right"] == 7 and c["pad_block/below"] == 11 and c["pad_block/corner"] == 1
    assert c["dc_pred/ix"] > 0 and c["dc_pred/iy"] > 0 and c["dc_pred/mx"] > 0 and c["dc_pred/my"] > 0
    c = cen("dc/ladder", "flat16", "420", 8, 8)
    assert c["pad_block/right"] == c["pad_block/below"] == c["pad_block/corner"] == 1


def test_code_tables_are_prefix_codes_of_at_most_16_bits():
    for family in ("symbols/cyclic", "wide", "quant/huge", "phase/tiny"):
        s = ed.case(family, "420", 85, 53).symbols
        for kind in ("flat16", "skewed"):
            depth, code = ed.tables(kind, s.hist)       # (tables() checks the prefix property of every table)
            assert depth.max() == 16 and depth[1, :, 0xf0].tolist() == [16] * 3 and depth[1, :, 0].tolist() == [16] * 3
        depth, code = ed.tables("skewed", s.hist)
        assert code[1, 0, 0xf0] == 0xffff and code[1, 0, 0] == 0xfffe
        others = np.where(np.isin(np.arange(256), (0, 0xf0)), 0, s.hist[1, 0])
        if others.any():                                  # a depth-16 code on the most frequent symbol
            assert depth[1, 0, np.argmax(others)] == 16 and code[1, 0, np.argmax(others)] == 0xfffd
        else:
            assert family in ("quant/huge", "phase/tiny")
    s = ed.case("symbols/cyclic", "444", 448, 296).symbols
    depth, _ = ed.tables("skewed", s.hist)
    assert set(depth[0].ravel()) | set(depth[1].ravel()) >= set(range(1, 9)) | {16}
    with pytest.raises(AssertionError):
        ed.check_prefix_code(np.array([1, 2] + [0] * 254), np.array([1, 2] + [0] * 254), np.arange(256) < 2)   # 1 / 10
    with pytest.raises(AssertionError):
        ed.check_prefix_code(np.full(256, 17), np.zeros(256, np.int64), np.arange(256) < 1)


# --------------------------------------------------------------- the emulation build --
EMU_SMALL = [s for s in ed.SHAPES if s[1] * s[2] < 20000]
# the large shapes, where the emulation can afford them: the families whose condition needs many MCUs
EMU_LARGE = {"dense": [("444", 448, 296), ("420", 448, 296), ("gray", 448, 296)],
             "sparse": [("444", 448, 296), ("420", 448, 296)],
             "symbols/cyclic": [("420", 448, 296)],
             "wide": [("420", 448, 296)]}
EMU_HUGE = {("dense", "flat16"), ("sparse", "optimal")}     # 520 x 512: the statistics kernel's second trip


@pytest.fixture(scope="module")
def contexts(L):
    cache = pc.ContextCache(L)
    yield cache
    cache.close()


@pytest.mark.parametrize("kind", ed.KINDS)
@pytest.mark.parametrize("family", list(ed.FAMILIES))
def test_emulation(contexts, family, kind):
    shapes = EMU_SMALL + EMU_LARGE.get(family, []) + ([("444", 520, 512)] if (family, kind) in EMU_HUGE else [])
    pc.case_entropy_domain(contexts, host_emu(), family, kind, shapes)


def test_emulation_keep_across_scans(L):
    pc.case_entropy_keep_across_scans(L, host_emu())


def test_emulation_scan_probe(L):
    """(The emulation runs the workgroups one after the other: every look-back finds the inclusive prefix in the
    nearest tile, and a repeat is the same run again.)"""
    pc.case_scan_probe(L, repeats=1)
    with pytest.raises(Exception):
        L.probe_scan_offsets(np.zeros(4, np.uint32), [5])
    with pytest.raises(Exception):
        L.probe_scan_offsets(np.zeros(4, np.uint32), [0])


if __name__ == "__main__":
    rec = derive()[0]
    if "--write" in sys.argv:
        json.dump(rec, open(GOLDEN, "w"), indent=1, sort_keys=True)
        print("wrote", GOLDEN)
    else:
        print(json.dumps(rec, indent=1, sort_keys=True))
