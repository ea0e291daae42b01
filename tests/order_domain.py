"""Phase B's device side (guetzli_amd/csrc/gz_kernels_order.h through api/entry_phaseb.h) on state built for its arms.

A plain numpy restatement -- float32 and float64 exactly where the reference promotes -- of
  ComputeBlockErrorAdjustmentWeights from block maxima (butteraugli_comparator.cc:521-557; 2x2 grouping for factor 2),
  the construction loop of the global order (processor.cc:636-663) with blocks_to_change and the count below `limit`,
  the update of max_block_error (processor.cc:754-756),
  the whole-block steps (processor.cc:704-736) with Quantize (quantize.h:24-29) and the precious rule,
  the change of the AC statistics (through entropy_domain.symbolize, which is pinned to the writers),
  the position the device derives for its descent (gz_kernels_order.h: desc_load),
and the families of inputs the kernels are run on.  Every restatement counts the arm each input takes (`census`);
tests/test_order_domain.py pins the restatements and records the counts, tests/parity_cases.py runs the families through
the C ABI (the emulation build there, the device in tests/test_order_gpu.py).  Nothing here has a tolerance.

The state is installed with the three hooks gz_probe_set_block_max / gz_probe_set_search / gz_probe_order_state; every
kernel runs through the production entry points.

Outside the domain: direction -1 with next_cand > cnt (the reference reads the NEXT block's candidates there, the device
its own stride of 192: undefined in both); Quantize where raw + delta leaves int16 is kept (both wrap the same way).
"""
import numpy as np

import entropy_domain as ed

F32 = np.float32
F64 = np.float64
# gz_create's target: float(td) lies ABOVE td = target * 0.97 for the first and BELOW it for the second (with
# target_mul 1.0 td is the float itself); 0.971769 is ButteraugliScoreForQuality(95)
TARGETS = (0.971769, 0.9)
MULS = (1.0, 0.97)
RADII = (1, 2, 3, 4)
BIG = (1040, 1040)      # 130 x 130 = 16 900 blocks: 67 groups of 256 (k_order_fill's second trip), per = 3 in the steps


def bits32(x):
    return np.asarray(x, F32).view(np.uint32).astype(np.int64)


def ulps(x, k):
    """x moved by k float32 steps (positive finite x)."""
    return (np.asarray(x, F32).view(np.uint32).astype(np.int64) + k).astype(np.uint32).view(F32)


def count(census, key, n=1):
    if census is not None:
        census[key] = census.get(key, 0) + int(n)


# =============================================================== the grids =========
class Grid:
    """A context size, its frame and the component mask of a search: the search grid (gw x gh) over the 8x8 blocks."""

    def __init__(self, w, h, layout="444", mask=7):
        assert (layout, mask) in (("444", 7), ("444", 1), ("420", 1), ("420", 6))
        self.w, self.h, self.layout, self.mask = w, h, layout, mask
        self.bw, self.bh = (w + 7) // 8, (h + 7) // 8
        self.nb = self.bw * self.bh
        self.cbw, self.cbh = (w + 15) // 16, (h + 15) // 16
        self.nbc = self.cbw * self.cbh
        self.factor = 2 if (layout == "420" and mask == 6) else 1
        self.gw, self.gh = (self.cbw, self.cbh) if self.factor == 2 else (self.bw, self.bh)
        self.gn = self.gw * self.gh
        self.comps = [c for c in range(3) if (mask >> c) & 1]
        self.coff = [0, self.nb, self.nb + self.nbc] if layout == "420" else [0, self.nb, 2 * self.nb]
        self.nblk = self.nb + 2 * self.nbc if layout == "420" else 3 * self.nb

    @property
    def name(self):
        return f"{self.layout}/{self.mask} {self.w}x{self.h}"


def grid_of_blocks(gw, gh):
    return Grid(8 * gw, 8 * gh)


# ================================================== the weights (butteraugli_comparator.cc) ====
def group_max(bmax8, g):
    """The maxima over the search grid's areas (:505-520): the 8x8 maxima themselves, or 2x2 groups of them."""
    m = np.asarray(bmax8, F32).reshape(g.bh, g.bw)
    if g.factor == 1:
        return m.copy()
    out = np.zeros((g.gh, g.gw), F32)
    for dy in (0, 1):
        for dx in (0, 1):
            sub = m[dy::2, dx::2]
            out[:sub.shape[0], :sub.shape[1]] = np.maximum(out[:sub.shape[0], :sub.shape[1]], sub)
    return out


def _shifted(a, dy, dx, fill):
    gh, gw = a.shape
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, gh), slice(0, gh - dy)) if dy >= 0 else (slice(0, gh + dy), slice(-dy, gh))
    xs, xd = (slice(dx, gw), slice(0, gw - dx)) if dx >= 0 else (slice(0, gw + dx), slice(-dx, gw))
    if abs(dy) < gh and abs(dx) < gw:
        out[yd, xd] = a[ys, xs]
    return out


def _hug(census, key, x, thr64, le):
    """Comparison `x <= thr` of float32 x promoted to double: each side, and how many operands sit within one float32
    step of the threshold's nearest float on each side."""
    near = np.abs(bits32(x) - bits32(F32(thr64))) <= 1
    count(census, f"w/{key}/le", le.sum())
    count(census, f"w/{key}/gt", (~le).sum())
    count(census, f"w/{key}/le_hug", (le & near).sum())
    count(census, f"w/{key}/gt_hug", (~le & near).sum())


def weights(gmax, target, direction, r, target_mul, use_distmap=True, census=None):
    """ComputeBlockErrorAdjustmentWeights on the search grid's maxima [gh][gw] (weights zeroed first, as the driver
    does): float32 [gh * gw]."""
    gh, gw = gmax.shape
    td = F64(F32(target)) * F64(target_mul)             # double target_distance = float * double
    tdf = F32(td)                                       # max_local_dist starts as static_cast<float>(target_distance)
    m = np.asarray(gmax, F32) if use_distmap else np.zeros((gh, gw), F32)
    count(census, "w/tdf_above_td" if F64(tdf) > td else "w/tdf_below_td" if F64(tdf) < td else "w/tdf_equals_td")
    count(census, "w/nodistmap" if not use_distmap else "w/distmap")
    count(census, "w/radius_covers_grid" if r >= max(gw, gh) else "w/radius_covers_one_axis" if r >= min(gw, gh) else
          "w/radius_inside_grid")
    local = np.full((gh, gw), tdf, F32)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            local = np.maximum(local, _shifted(m, dy, dx, F32(0)))
    own64, loc64 = m.astype(F64), local.astype(F64)
    yy, xx = np.mgrid[0:gh, 0:gw]
    clipped = (yy - r < 0) | (xx - r < 0) | (yy + r >= gh) | (xx + r >= gw)
    if direction > 0:
        a = own64 <= td
        b = loc64 <= F64(1.1) * td
        _hug(census, "own", m, td, a)
        _hug(census, "local", local, F64(1.1) * td, b)
        return (a & b).astype(F32).reshape(-1)
    thr = (1 - F64(0.5)) * td + F64(0.5) * loc64
    cold = own64 <= thr
    if census is not None:
        near = np.abs(bits32(m) - bits32(thr.astype(F32))) <= 1
        count(census, "w/mix/le", cold.sum())
        count(census, "w/mix/gt", (~cold).sum())
        count(census, "w/mix/le_hug", (cold & near).sum())
        count(census, "w/mix/gt_hug", (~cold & near).sum())
    hot = ~cold
    w = np.zeros((gh, gw), F32)
    dmin = np.full((gh, gw), r + 1, np.int64)
    for d in range(r, -1, -1):                          # the nearest hot block gives the largest 1 / (d + 1)
        reach = np.zeros((gh, gw), bool)
        for dy in range(-d, d + 1):
            for dx in range(-d, d + 1):
                reach |= _shifted(hot, dy, dx, False)
        w = np.where(reach, F32(1.0) / (F32(d) + F32(1.0)), w).astype(F32)
        dmin = np.where(reach, d, dmin)
    if census is not None:
        for d in range(5):
            count(census, f"w/cheb/{d}/clipped", ((dmin == d) & (dmin <= r) & clipped).sum())
            count(census, f"w/cheb/{d}/full", ((dmin == d) & (dmin <= r) & ~clipped).sum())
        count(census, "w/cheb/none/clipped", ((dmin > r) & clipped).sum())
        count(census, "w/cheb/none/full", ((dmin > r) & ~clipped).sum())
    return w.reshape(-1)


def weights_of(g, bmax8, target, direction, r, target_mul, use_distmap=True, census=None):
    if census is not None and use_distmap:
        ragged = g.factor == 2 and (g.bw % 2 or g.bh % 2)
        count(census, "w/group/ragged" if ragged else "w/group/pairs" if g.factor == 2 else "w/group/none")
    return weights(group_max(bmax8, g), target, direction, r, target_mul, use_distmap, census)


def distmap_of(bmax8, g, rng=None):
    """A distance map [h][w] whose 8x8 maxima are bmax8: one pixel of every block carries the maximum."""
    dm = np.zeros((g.h, g.w), F32)
    m = np.asarray(bmax8, F32).reshape(g.bh, g.bw)
    for by in range(g.bh):
        for bx in range(g.bw):
            ys, xs = min(8, g.h - 8 * by), min(8, g.w - 8 * bx)
            k = (by * 31 + bx * 7) % (ys * xs)
            dm[8 * by + k // xs, 8 * bx + k % xs] = m[by, bx]
    return dm


# ==================================================== the construction loop (processor.cc:636-663) ====
FILL_LANES = 16
ORDER_GROUP = 256


def build_order(off, err, next_cand, max_err, wgt, direction, limit=None, census=None):
    """-> (blocks int32, vals float32, blocks_to_change, entries with val < limit)."""
    off = np.asarray(off, np.int64)
    cnt = np.diff(off)
    at = np.asarray(next_cand, np.int64)
    wgt, me, err = np.asarray(wgt, F32), np.asarray(max_err, F32), np.asarray(err, F32)
    raw = cnt - at if direction > 0 else at
    assert direction > 0 or (at <= cnt).all(), "outside the domain (module docstring)"
    assert (at >= 0).all() and (cnt <= 192).all()
    live = wgt != 0
    n = np.where(live, np.maximum(raw, 0), 0)
    total = int(n.sum())
    blocks = np.repeat(np.arange(cnt.size), n)
    j = np.arange(total) - np.repeat(np.cumsum(n) - n, n)
    pos = off[blocks] + (at[blocks] + j if direction > 0 else at[blocks] - 1 - j)
    e = err[pos] if total else np.zeros(0, F32)
    with np.errstate(all="ignore"):
        vals = ((e - me[blocks]) / wgt[blocks] if direction > 0 else (me[blocks] - e) / wgt[blocks]).astype(F32)
    below = int((vals < F32(limit)).sum()) if limit is not None else 0
    if census is not None:
        count(census, "fill/n/0", (live & (n == 0)).sum())
        count(census, "fill/n/1to16", ((n >= 1) & (n <= FILL_LANES)).sum())
        count(census, "fill/n/17to32", ((n > FILL_LANES) & (n <= 2 * FILL_LANES)).sum())
        count(census, "fill/n/gt32", (n > 2 * FILL_LANES).sum())
        for k in (16, 17, 32, 33):
            count(census, f"fill/n/eq{k}", (n == k).sum())
        count(census, "fill/weight_zero", (~live).sum())
        count(census, "fill/clamp", (live & (raw < 0)).sum())
        ngroups = -(-cnt.size // ORDER_GROUP)
        count(census, "fill/group_trips/2" if ngroups > 64 else "fill/group_trips/1")
        gsum = np.add.reduceat(n, np.arange(0, cnt.size, ORDER_GROUP))
        count(census, "fill/group/empty_before_live", sum(1 for i in range(ngroups) if gsum[i] == 0 and gsum[i + 1:].any()))
        count(census, "fill/group/partial_last", int(cnt.size % ORDER_GROUP != 0))
        count(census, "fill/group/full_last", int(cnt.size % ORDER_GROUP == 0))
        count(census, "fill/val/negative", (vals < 0).sum())
        count(census, "fill/val/zero", (vals == 0).sum())
        count(census, "fill/val/positive", (vals > 0).sum())
        tiny = F32(1.1754944e-38)
        count(census, "fill/val/denormal_operands", ((np.abs(e) < tiny) & (e != 0)).sum())
        if limit is not None:
            count(census, "fill/below/lt", (vals < F32(limit)).sum())
            count(census, "fill/below/eq", (vals == F32(limit)).sum())
            count(census, "fill/below/gt", (vals > F32(limit)).sum())
        else:
            count(census, "fill/below/not_counted")
    return blocks.astype(np.int32), vals, int((n > 0).sum()), below


def advance(max_err, wgt, thr, direction):
    """max_block_error[i] += block_weight[i] * val_threshold * direction: float product, times the int."""
    return (np.asarray(max_err, F32) + (np.asarray(wgt, F32) * F32(thr)) * F32(direction)).astype(F32)


# =========================================================== the steps (processor.cc:704-736) ====
def quantize(raw, q, census=None):
    """Quantize (quantize.h:24-29) with its coeff_t (int16) delta and result."""
    raw = np.asarray(raw, np.int64)
    q = np.asarray(q, np.int64)
    r = np.fmod(raw, q)                                 # C++ %: the sign of the dividend
    up, down = 2 * r > q, -2 * r > q
    delta = np.where(up, q - r, np.where(down, -q - r, -r)).astype(np.int16).astype(np.int64)
    if census is not None:
        count(census, "quantize/round_up", up.sum())
        count(census, "quantize/round_down_negative", (~up & down).sum())
        count(census, "quantize/towards_zero", (~up & ~down).sum())
        count(census, "quantize/tie_2r_eq_q", (2 * r == q).sum())
        count(census, "quantize/tie_neg_2r_eq_q", (-2 * r == q).sum())
        count(census, "quantize/q_gt_abs_raw", (q > np.abs(raw)).sum())
        count(census, "quantize/q_is_1", (q == 1).sum())
    return (raw + delta).astype(np.int16)


LOW_CORNER = np.array([(i & 7) < 3 and i < 24 for i in range(64)])
HF = ~LOW_CORNER & (np.arange(64) >= 3)


def sum_of_hf(orig_block):
    return int(np.abs(np.asarray(orig_block, np.int64))[HF].sum())


HIST_GRID = 2048


def apply_steps(g, coeffs, orig, q, off, idx, next_cand, direction, blocks, counts, census=None):
    """The candidate after entry i advanced block blocks[i] by counts[i] steps (frame-layout arrays [nblk][64])."""
    out = np.asarray(coeffs, np.int16).reshape(-1, 64).copy()
    og = np.asarray(orig, np.int16).reshape(-1, 64)
    q = np.asarray(q, np.int64).reshape(3, 64)
    n = len(blocks)
    if census is not None:
        grid = min(-(-n // 4), HIST_GRID)
        per = -(-n // (grid * 4)) if n else 0
        count(census, "steps/per/1" if per == 1 else "steps/per/2" if per == 2 else "steps/per/3plus")
        count(census, "steps/wavefront/live", n)
        count(census, "steps/wavefront/not_live", grid * 4 * per - n)
        count(census, "steps/count/gt64", (np.asarray(counts) > 64).sum())
        count(census, "steps/count/le64", (np.asarray(counts) <= 64).sum())
    blocks, counts = np.asarray(blocks, np.int64), np.asarray(counts, np.int64)
    off, idx, nx = np.asarray(off, np.int64), np.asarray(idx, np.int64), np.asarray(next_cand, np.int64)
    bb = np.repeat(blocks, counts)                                   # one row per step
    j = np.arange(bb.size) - np.repeat(np.cumsum(counts) - counts, counts)
    p = nx[bb] + j if direction > 0 else nx[bb] - 1 - j
    assert bb.size == 0 or ((p >= 0) & (p < (off[bb + 1] - off[bb]))).all(), "a step outside the block's candidates"
    ix = idx[off[bb] + p]
    c, k = ix // 64, ix % 64
    assert np.isin(c, g.comps).all()
    row = np.asarray(g.coff, np.int64)[c] + bb
    raw = og[row, k].astype(np.int64)
    newval = np.zeros(bb.size, np.int64) if direction > 0 else quantize(raw, q[c, k], census).astype(np.int64)
    hf = np.abs(og[row].astype(np.int64))[:, HF].sum(axis=1)
    lim = np.where(hf < 60, 4, 8)
    k18 = (k == 1) | (k == 8)
    precious = k18 & (np.abs(raw) >= lim)
    if census is not None:
        count(census, "steps/precious/other_k", (~k18).sum())
        count(census, "steps/precious/newval_nonzero", (k18 & (newval != 0)).sum())
        for L in (4, 8):
            sel = k18 & (newval == 0) & (lim == L)
            count(census, f"steps/precious/limit{L}/yes", (sel & precious).sum())
            count(census, f"steps/precious/limit{L}/no", (sel & ~precious).sum())
    write = ~precious | (newval != 0)
    out[row[write], k[write]] = newval[write].astype(np.int16)
    return out


def ac_hist_blocks(blocks, jq_c):
    """AC statistics [256] of some blocks of one component (BuildACHistograms) under its quantiser: a block's AC
    symbols depend on nothing but the block, so they are counted as a strip of single-block MCUs."""
    blocks = np.asarray(blocks, np.int16).reshape(-1, 64).copy()
    if not blocks.shape[0]:
        return np.zeros(256, np.int64)
    blocks[:, 0] = 0                                  # (the DC symbols are not part of it)
    q3 = np.ones((3, 64), np.int64)
    q3[0] = jq_c
    return ed.symbolize(ed.Geom("gray", 8 * blocks.shape[0], 8), [blocks], q3).hist[1, 0].astype(np.int64)


def ac_hist(g, coeffs, jq):
    """AC statistics [3][256] of a whole frame: entropy_domain.symbolize on its own geometry (padding blocks included:
    the same before and after any step)."""
    geom = ed.Geom(g.layout, g.w, g.h)
    co = np.asarray(coeffs, np.int16).reshape(-1, 64)
    first = np.concatenate([[0], np.cumsum(geom.array_blocks)])
    blocks = [co[first[c]:first[c + 1]].copy() for c in range(3)]
    for b in blocks:
        b[:, 0] = 0
    return ed.symbolize(geom, blocks, jq).hist[1].astype(np.int64)


def component_rows(g, c):
    return g.coff[c], g.coff[c] + (g.nb if (c == 0 or g.layout == "444") else g.nbc)


def hist_delta(g, before, after, jq, census=None):
    before, after = np.asarray(before).reshape(-1, 64), np.asarray(after).reshape(-1, 64)
    jq = np.asarray(jq, np.int64).reshape(3, 64)
    d = np.zeros((3, 256), np.int64)
    for c in range(3):                                # the blocks that changed: the others cancel
        lo, hi = component_rows(g, c)
        ch = lo + np.flatnonzero((before[lo:hi] != after[lo:hi]).any(axis=1))
        d[c] = ac_hist_blocks(after[ch], jq[c]) - ac_hist_blocks(before[ch], jq[c])
    if census is not None:
        for name, s in (("zrl", 0xf0), ("eob", 0)):
            count(census, f"steps/{name}/more", (d[:, s] > 0).sum())
            count(census, f"steps/{name}/fewer", (d[:, s] < 0).sum())
        count(census, "steps/delta/zero" if not d.any() else "steps/delta/nonzero")
    return d


# ============================================= the descent's position (gz_kernels_order.h: desc_load) ====
def derived_last(per_block, btc, n, census=None):
    """min_coeffs_to_change = float product, truncated (processor.cc:685-687); capped at the order's last position;
    down to a multiple of 10 (the codes are refreshed every 10th step); the position before it."""
    assert n > 0
    mc = int(F32(per_block) * F32(btc))
    exact = int(F64(F32(per_block)) * btc)
    mc = max(mc, 0)
    last_needed = min(mc, n - 1)
    fast_until = last_needed // 10 * 10
    last = fast_until - 1 if fast_until else 0
    count(census, "last/capped" if mc > n - 1 else "last/uncapped")
    count(census, "last/zero" if not fast_until else "last/multiple_of_10" if last_needed % 10 == 0 else "last/rounded_down")
    count(census, "last/float_product_differs", mc != exact)
    count(census, "last/float_product_exact", mc == exact)
    return last


def btc_values(per_block, limit):
    """0..60, and every blocks_to_change whose product with per_block lands within one of a multiple of 10."""
    b = np.arange(limit + 1)
    mc = (F32(per_block) * b.astype(F32)).astype(np.int64)
    near = np.isin(mc % 10, (9, 0, 1)) & (mc >= 9)
    return sorted(set(range(0, min(60, limit) + 1)) | set(b[near].tolist()))


# ================================================================== the families ==========
class WeightCase:
    """Block maxima (8x8 blocks of the context) for gz_order_build_auto's weights on grid g at gz_create's target."""

    def __init__(self, family, g, target, bmax8, use_distmap=True):
        self.family, self.g, self.target, self.use_distmap = family, g, target, use_distmap
        self.bmax8 = np.ascontiguousarray(bmax8, F32).reshape(-1)
        assert self.bmax8.size == g.nb and (self.bmax8 >= 0).all()

    def reference(self, direction, r, mul, census=None):
        return weights_of(self.g, self.bmax8, self.target, direction, r, mul, self.use_distmap, census)


WEIGHT_GRIDS = [grid_of_blocks(1, 1), grid_of_blocks(9, 1), grid_of_blocks(1, 9), grid_of_blocks(17, 13),
                grid_of_blocks(16, 16), grid_of_blocks(17, 16),
                Grid(136, 104, "420", 6), Grid(24, 24, "420", 6), Grid(136, 104, "420", 1), Grid(128, 128, "420", 6)]
HUG_STEPS = (-2, -1, 0, 1, 2)


def _td(target, mul):
    return F64(F32(target)) * F64(mul)


def _probe_sites(g, spacing):
    """Blocks of the 8x8 grid far enough apart, the corners and edges first."""
    ys = sorted({0, g.bh - 1} | set(range(0, g.bh, spacing)))
    xs = sorted({0, g.bw - 1} | set(range(0, g.bw, spacing)))
    return [(y, x) for y in ys for x in xs]


def fam_hug(which):
    def make(g, target, rng):
        """Maxima at nextafter steps around the threshold of both target_mul values; several maps, since a probe's
        neighbourhood of radius 4 covers a small grid."""
        maps = []
        for mul in MULS:
            td = _td(target, mul)
            for rot in range(len(HUG_STEPS)):
                m = np.zeros((g.bh, g.bw), F32)
                f = 2 if g.factor == 2 else 1
                sites = _probe_sites(g, 3 * f)
                if max(g.gw, g.gh) < 5:               # one neighbourhood holds the whole grid: one probe per map
                    sites = [sites[rot % len(sites)]]
                for i, (y, x) in enumerate(sites):
                    k = HUG_STEPS[(i + rot) % len(HUG_STEPS)]
                    if which == "own":
                        m[y, x] = ulps(F32(td), k)
                    elif which == "local":            # a neighbour at 1.1 td: the cold blocks around it see it as `local`
                        m[y, x] = ulps(F32(F64(1.1) * td), k)
                    else:                             # a hot block M and, beside it, one at 0.5 td + 0.5 M
                        M = F32(td * (1.5 + 0.25 * (i % 3)))
                        m[y, x] = M
                        thr = F32((1 - F64(0.5)) * td + F64(0.5) * F64(M))
                        x2 = x + f if x + f < g.bw else x - f
                        if 0 <= x2 < g.bw and m[y, x2] == 0:
                            m[y, x2] = ulps(thr, k)
                        elif g.bh > f:                # (a grid one block wide: below or above)
                            y2 = y + f if y + f < g.bh else y - f
                            if 0 <= y2 < g.bh and m[y2, x] == 0:
                                m[y2, x] = ulps(thr, k)
                if which == "mix" and rot == 0:       # ... and alone, where `local` is the block's own maximum
                    m2 = np.zeros((g.bh, g.bw), F32)
                    for i, (y, x) in enumerate(sites):
                        m2[y, x] = ulps(F32(td), HUG_STEPS[i % len(HUG_STEPS)])
                    maps.append(m2)
                maps.append(m)
        return maps
    return make


def fam_lone(g, target, rng):
    hot = F32(3.0 * target)
    sites = sorted({(0, 0), (0, g.bw - 1), (g.bh - 1, 0), (g.bh - 1, g.bw - 1), (0, g.bw // 2), (g.bh // 2, 0),
                    (g.bh - 1, g.bw // 2), (g.bh // 2, g.bw - 1), (g.bh // 2, g.bw // 2)})
    maps = []
    for y, x in sites:
        m = np.full((g.bh, g.bw), F32(0.25 * target), F32)
        m[y, x] = hot
        maps.append(m)
    return maps


def fam_pair(g, target, rng):
    maps = []
    for dy, dx in ((0, 3), (3, 0), (2, 5), (4, 4), (0, 1)):
        m = np.full((g.bh, g.bw), F32(0.25 * target), F32)
        y, x = g.bh // 3, g.bw // 3
        m[y, x] = F32(3.0 * target)
        m[min(y + dy, g.bh - 1), min(x + dx, g.bw - 1)] = F32(4.0 * target)
        maps.append(m)
    return maps


def fam_all_cold(g, target, rng):
    return [np.full((g.bh, g.bw), F32(0.5 * target), F32), np.zeros((g.bh, g.bw), F32)]


def fam_all_hot(g, target, rng):
    return [np.full((g.bh, g.bw), F32(2.0 * target), F32),
            (F32(2.0 * target) + rng.random((g.bh, g.bw)).astype(F32)).astype(F32)]


def fam_nodistmap(g, target, rng):
    return [np.full((g.bh, g.bw), F32(2.0 * target), F32)]


def fam_random(g, target, rng):
    """Maxima spread around the target: every arm at once, as a photograph's map gives them."""
    return [(rng.random((g.bh, g.bw)) ** 2 * 2.2 * target).astype(F32) for _ in range(2)]


WEIGHT_FAMILIES = {"hug/own": fam_hug("own"), "hug/local": fam_hug("local"), "hug/mix": fam_hug("mix"),
                   "lone": fam_lone, "pair": fam_pair, "all_cold": fam_all_cold, "all_hot": fam_all_hot,
                   "nodistmap": fam_nodistmap, "random": fam_random}


def weight_cases(family, g, target):
    rng = np.random.default_rng(sum(map(ord, family + g.name)) * 7919 + int(target * 1000))
    return [WeightCase(family, g, target, m, use_distmap=family != "nodistmap")
            for m in WEIGHT_FAMILIES[family](g, target, rng)]


# --------------------------------------------------------------- construction -----
class OrderCase:
    """Candidates (CSR), next_cand, max_block_error, and block maxima whose weights (direction, r, mul) the four entry
    points build the order with."""

    def __init__(self, family, g, target, bmax8, direction, r, mul, off, err, next_cand, max_err, limit):
        self.family, self.g, self.target = family, g, target
        self.bmax8 = np.ascontiguousarray(bmax8, F32).reshape(-1)
        self.direction, self.r, self.mul = direction, r, mul
        self.off = np.ascontiguousarray(off, np.int32)
        self.err = np.ascontiguousarray(err, F32)
        self.idx = (np.arange(self.err.size) % 63 + 1).astype(np.uint8)       # (not read by the order)
        self.next_cand = np.ascontiguousarray(next_cand, np.int32)
        self.max_err = np.ascontiguousarray(max_err, F32)
        self.limit = limit
        assert self.off.size == g.gn + 1 and self.next_cand.size == g.gn == self.max_err.size

    def weights(self, census=None):
        return weights_of(self.g, self.bmax8, self.target, self.direction, self.r, self.mul, True, census)

    def reference(self, census=None):
        return build_order(self.off, self.err, self.next_cand, self.max_err, self.weights(census), self.direction,
                           self.limit, census)


FILL_EDGES = (0, 1, 15, 16, 17, 31, 32, 33, 48, 49, 189, 192)
ORDER_GRIDS = {255: grid_of_blocks(17, 15), 256: grid_of_blocks(16, 16), 257: grid_of_blocks(257, 1),
               1023: grid_of_blocks(33, 31), 16900: Grid(*BIG), 221: grid_of_blocks(17, 13)}


def _bmax_for(g, target, direction, kind, rng):
    """Block maxima that give: "ones" weight 1 everywhere; "alternate" weight 0 / 1 by turns ("up": maxima between td
    and 1.1 td are cold themselves and leave their neighbours alone); "groups" whole groups of 256 blocks at weight 0;
    "falloff" (down) hot blocks eight apart: weights 1, 1/2 .. 1/5."""
    m = np.zeros(g.nb, F32)
    if kind == "ones":
        if direction < 0:
            m[:] = F32(3.0 * target)
    elif kind == "alternate":
        assert direction > 0
        m[1::2] = F32(1.05 * target)
    elif kind == "groups":
        if direction > 0:
            m[:] = F32(3.0 * target)                                   # cold-less: weight 0 ...
            k = 4 if g.nb > 4096 else 1                                # ... but every other run of k groups
            for grp in range(-(-g.nb // 256)):
                if (grp // k) % 2 == 0:
                    m[grp * 256:(grp + 1) * 256] = 0
            # (the blocks that see a hot one within the radius drop out too: whole groups and partial ones)
        else:
            m[:] = F32(0.25 * target)
            m[(g.bh // 2) * g.bw + g.bw // 2] = F32(3.0 * target)      # one hot block: everything beyond r is 0
    elif kind == "falloff":
        assert direction < 0
        m[:] = F32(0.25 * target)
        mm = m.reshape(g.bh, g.bw)
        mm[::10, ::10] = F32(3.0 * target)
    return m


def _csr(counts, rng, lo=0.0, hi=2.0):
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    err = (lo + (hi - lo) * rng.random(int(off[-1]))).astype(F32)
    return off, err


def order_cases(family, target=TARGETS[0]):
    rng = np.random.default_rng(sum(map(ord, family)) * 104729)
    out = []

    def add(g, direction, kind, counts, next_cand, err=None, max_err=None, limit=None, r=4, mul=1.0, off=None):
        if off is None:
            off, e2 = _csr(counts, rng)
            err = e2 if err is None else err
        me = np.zeros(g.gn, F32) if max_err is None else max_err
        out.append(OrderCase(family, g, target, _bmax_for(g, target, direction, kind, rng), direction, r, mul, off, err,
                             next_cand, me, limit))
    if family == "fill/edges":
        g = ORDER_GRIDS[221]
        E = np.array(FILL_EDGES)
        for direction in (1, -1):
            for mode in ("at0", "atcnt", "between"):
                n = E[np.arange(g.gn) % E.size]                       # the entries each block is to give
                if mode == "at0":                                     # up: all of cnt from 0; down: nothing applied yet
                    cnt, at = (n, np.zeros_like(n)) if direction > 0 else (n, np.zeros_like(n))
                elif mode == "atcnt":                                 # up: nothing left; down: all of cnt applied
                    cnt, at = n, n
                else:
                    extra = (np.arange(g.gn) * 7) % 4
                    cnt = np.minimum(n + extra, 192)
                    at = cnt - n if direction > 0 else n
                add(g, direction, "ones", cnt, at, limit=1.0, max_err=(rng.random(g.gn) * 0.5).astype(F32))
    elif family == "fill/overrun":
        g = ORDER_GRIDS[221]
        cnt = rng.integers(0, 40, g.gn)
        at = cnt + rng.integers(-3, 4, g.gn)
        at[::5] = cnt[::5] + 150
        add(g, 1, "ones", cnt, np.clip(at, 0, 400), limit=1.0)
    elif family == "groups":
        for nb in (255, 256, 257, 1023, 16900):
            g = ORDER_GRIDS[nb]
            cnt = rng.integers(0, 6, g.gn) if nb == 16900 else rng.integers(0, 40, g.gn)
            for direction, kind in ((1, "ones"), (1, "alternate"), (1, "groups"), (-1, "groups"), (-1, "falloff")):
                at = rng.integers(0, 1000, g.gn) % (cnt + 1)
                add(g, direction, kind, cnt, at, limit=None if kind == "alternate" else 0.5,       # (count_below = 0)
                    r=1 if kind == "groups" and direction > 0 else 4)
    elif family == "ties":
        g = ORDER_GRIDS[256]
        cnt = rng.integers(0, 50, g.gn)
        four = np.array([0.25, 0.5, 0.75, 1.0], F32)
        for direction, kind in ((1, "ones"), (-1, "falloff")):
            off, _ = _csr(cnt, rng)
            err = four[rng.integers(0, 4, int(off[-1]))]
            me = np.full(g.gn, F32(0.25), F32)
            at = rng.integers(0, 1000, g.gn) % (cnt + 1)
            # limit equal to a val the order holds: (0.75 - 0.25) / 1 "up", (0.25 - 0.5) / (1/2) = -0.5 "down"
            add(g, direction, kind, cnt, at, err=err, max_err=me, limit=0.5 if direction > 0 else -0.5, off=off)
    elif family == "signs":
        g = ORDER_GRIDS[255]
        cnt = rng.integers(1, 30, g.gn)
        for direction, kind in ((1, "ones"), (-1, "falloff")):
            off, err = _csr(cnt, rng)
            me = np.full(g.gn, F32(1.0), F32)
            err[::3] = F32(1.0)                                       # equal to max_err: val = +0 or -0
            at = rng.integers(0, 1000, g.gn) % (cnt + 1)
            add(g, direction, kind, cnt, at, err=err, max_err=me, limit=0.0, off=off)
    elif family == "small":
        g = ORDER_GRIDS[256]
        cnt = rng.integers(1, 30, g.gn)
        off, _ = _csr(cnt, rng)
        tiny = np.float32(1.1754944e-38)
        err = (rng.random(int(off[-1])).astype(F32) * tiny).astype(F32)            # denormal
        me = (rng.random(g.gn).astype(F32) * tiny * F32(0.5)).astype(F32)
        at = rng.integers(0, 1000, g.gn) % (cnt + 1)
        add(g, -1, "falloff", cnt, at, err=err, max_err=me, limit=float(tiny) * 0.25, off=off)     # weights 1/3, 1/5
        add(g, 1, "ones", cnt, at, err=err, max_err=me, limit=float(tiny) * 0.25, off=off)
    else:
        raise KeyError(family)
    return out


ORDER_FAMILIES = ("fill/edges", "fill/overrun", "groups", "ties", "signs", "small")

# --------------------------------------------------------------------- advance -----
ADVANCE_FAMILIES = ("advance/fused", "advance/escalate", "advance/twice", "advance/replaced")


# ----------------------------------------------------------------------- steps -----
class StepCase:
    """Original and candidate coefficients (frame layout [nblk][64]), a quantiser, candidates, and bulk-step calls."""

    def __init__(self, family, g, orig, cand, q, off, idx, calls, with_statistics=True):
        self.family, self.g = family, g
        self.orig = np.ascontiguousarray(orig, np.int16).reshape(g.nblk, 64)
        self.cand = np.ascontiguousarray(cand, np.int16).reshape(g.nblk, 64)
        self.q = np.ascontiguousarray(q, np.int32).reshape(3, 64)
        self.off = np.ascontiguousarray(off, np.int32)
        self.idx = np.ascontiguousarray(idx, np.uint8)
        self.calls = calls            # [(direction, next_cand [gn], blocks, counts, read_delta)]
        self.with_statistics = with_statistics
        comp = self.idx.astype(np.int64) // 64
        assert self.idx.size == 0 or (np.isin(comp, g.comps).all() and (self.idx % 64 != 0).all())
        for b in range(g.gn):                                        # a block's candidates are distinct coefficients
            s = self.idx[self.off[b]:self.off[b + 1]]
            assert len(set(s.tolist())) == s.size <= 192

    def layout(self, a):
        """The array as the context takes it."""
        return a.reshape(3, self.g.nb, 64) if self.g.layout == "444" else a

    def reference(self, census=None):
        """Per call: (coefficients after it, AC statistics change)."""
        cur, out = self.cand, []
        for direction, next_cand, blocks, counts, _ in self.calls:
            nxt = apply_steps(self.g, cur, self.orig, self.q, self.off, self.idx, next_cand, direction, blocks, counts, census)
            out.append((nxt, hist_delta(self.g, cur, nxt, self.q, census)))
            cur = nxt
        return out


STEP_Q = np.array([[1 + (3 * k + 5 * c) % 9 + (40 if k % 11 == 0 else 0) for k in range(64)] for c in range(3)], np.int32)
STEP_FAMILIES = ("precious/edges", "quantize/ties", "counts", "n/tails", "runs", "twice", "plain", "420")
NAT = ed.NATURAL


def _all_candidates(g, rng, per_comp=63):
    """Every AC coefficient of every component of the mask, shuffled per block: idx of one block."""
    ix = np.concatenate([c * 64 + 1 + rng.permutation(63)[:per_comp] for c in g.comps])
    return rng.permutation(ix).astype(np.uint8)


def _random_orig(g, rng, amp=40):
    o = rng.integers(-amp, amp + 1, (g.nblk, 64)).astype(np.int16)
    o[:, 0] = 0
    return o


def _requant(orig, q, g):
    out = orig.copy()
    for c in range(3):
        a, b = component_rows(g, c)
        out[a:b] = quantize(orig[a:b], q[c][None, :])
    return out


def step_cases(family):
    rng = np.random.default_rng(sum(map(ord, family)) * 15485863)
    g = Grid(136, 104)
    q = STEP_Q
    out = []
    if family == "precious/edges":
        # one block per (k, v, sum_of_hf, corner); the candidate is the unquantised original, so that a coefficient
        # the rule protects keeps a value no step writes
        rows = [(k, s * v, hf, corner) for k in (1, 8) for v in (3, 4, 7, 8) for s in (1, -1) for hf in (59, 60)
                for corner in (False, True)]
        orig = np.zeros((g.nblk, 64), np.int16)
        cnt = np.zeros(g.gn, np.int64)
        idx = []
        for b, (k, v, hf, corner) in enumerate(rows):
            for c in range(3):
                ob = orig[g.coff[c] + b]
                ob[3], ob[24] = hf - 20, -20                          # the included indices 3 and 24 carry the sum
                if corner:                                            # large values where the sum does not look
                    for j, ii in enumerate(i for i in (8, 9, 10, 16, 17, 18) if i != k):
                        ob[ii] = 2000 if j % 2 == 0 else -2000
                ob[k] = v
            ix = np.array([c * 64 + kk for c in range(3) for kk in (1, 8, 3, 24, 9)], np.uint8)
            idx.append(ix)
            cnt[b] = ix.size
        off = np.concatenate([[0], np.cumsum(cnt)])
        idx = np.concatenate(idx)
        q2 = np.ones((3, 64), np.int32)
        q2[:, 1], q2[:, 8] = 2, 5       # "down": Quantize(+-3, 2) = +-2, Quantize(+-3, 5) = +-5: written, precious or not
        q20 = q2.copy()
        q20[:, 1] = q20[:, 8] = 20      # "down": Quantize(v, 20) = 0 for every |v| <= 8: the rule decides again
        blocks = np.arange(len(rows), dtype=np.int32)
        counts = cnt[:len(rows)].astype(np.int32)
        full = cnt.astype(np.int32)
        for qq in (q2, q20):
            out.append(StepCase(family, g, orig, orig, qq, off, idx, [(1, np.zeros(g.gn, np.int32), blocks, counts, True)]))
            out.append(StepCase(family, g, orig, orig, qq, off, idx, [(-1, full, blocks, counts, True)]))
    elif family == "quantize/ties":
        # coefficient k of block b: raw chosen against q[k] so that 2r == q, 2r == q +- 1, negative, q > |raw|, q = 1
        qq = np.array([[1 if k % 7 == 0 else 2 + (k * 5 + c * 3) % 30 for k in range(64)] for c in range(3)], np.int32)
        orig = np.zeros((g.nblk, 64), np.int16)
        kinds = ("tie", "tie_plus", "tie_minus", "neg_tie", "neg_tie_plus", "neg_tie_minus", "small", "neg_small", "big")
        for b in range(g.gn):
            for c in range(3):
                for k in range(1, 64):
                    qv = int(qq[c, k])
                    kind = kinds[(b + k + c) % len(kinds)]
                    m = (b % 5) * qv
                    half = qv // 2
                    r = {"tie": half, "tie_plus": half + 1, "tie_minus": max(half - 1, 0), "neg_tie": -half,
                         "neg_tie_plus": -(half + 1), "neg_tie_minus": -max(half - 1, 0), "small": min(1, qv - 1),
                         "neg_small": -min(1, qv - 1), "big": 900 + b}[kind]
                    orig[g.coff[c] + b, k] = (m if r >= 0 else -m) + r
        cnt = np.full(g.gn, 189, np.int64)
        off = np.concatenate([[0], np.cumsum(cnt)])
        idx = np.concatenate([_all_candidates(g, rng) for _ in range(g.gn)])
        cand = np.zeros((g.nblk, 64), np.int16)                        # everything zeroed: "down" restores it all
        blocks = rng.permutation(g.gn).astype(np.int32)
        out.append(StepCase(family, g, orig, cand, qq, off, idx, [
            (-1, np.full(g.gn, 189, np.int32), blocks, np.full(g.gn, 189, np.int32), True)]))
    elif family == "counts":
        orig = _random_orig(g, rng)
        cnt = np.full(g.gn, 189, np.int64)
        off = np.concatenate([[0], np.cumsum(cnt)])
        idx = np.concatenate([_all_candidates(g, rng) for _ in range(g.gn)])
        cand = _requant(orig, q, g)
        blocks = np.arange(10, dtype=np.int32)
        counts = np.array([1, 63, 64, 65, 189, 1, 63, 64, 65, 189], np.int32)
        nc_up = np.zeros(g.gn, np.int32)
        nc_dn = np.full(g.gn, 189, np.int32)
        out.append(StepCase(family, g, orig, cand, q, off, idx, [(1, nc_up, blocks, counts, True)]))
        out.append(StepCase(family, g, orig, np.zeros_like(cand), q, off, idx, [(-1, nc_dn, blocks, counts, True)]))
    elif family == "n/tails":
        for gg, ns in ((g, (1, 3, 4, 5)), (Grid(*BIG), (8191, 8192, 8193, 16900))):
            orig = _random_orig(gg, rng)
            cnt = np.full(gg.gn, 6, np.int64)
            off = np.concatenate([[0], np.cumsum(cnt)])
            one = np.array([1, 8, 64 + 2, 128 + 9, 63, 64 + 63], np.uint8)
            idx = np.tile(one, gg.gn)
            cand = _requant(orig, q, gg)
            calls = []
            for i, n in enumerate(ns):
                direction = 1 if i % 2 == 0 else -1
                blocks = rng.permutation(gg.gn)[:n].astype(np.int32)
                counts = rng.integers(1, 4, n).astype(np.int32)
                nc = np.full(gg.gn, 0 if direction > 0 else 6, np.int32)
                calls.append((direction, nc, blocks, counts, True))
            out.append(StepCase(family, gg, orig, cand, q, off, idx, calls))
    elif family == "runs":
        # zig-zag positions: a lone coefficient at the end of a run of 16 / 32 / 48 zeros appears and disappears
        q1 = np.ones((3, 64), np.int32)
        orig = np.zeros((g.nblk, 64), np.int16)
        cnt = np.zeros(g.gn, np.int64)
        idx = []
        shapes = [(17,), (33,), (49,), (63,), (17, 34), (3, 63), (16, 32, 48), (5,)]
        for b in range(g.gn):
            zz = shapes[b % len(shapes)]
            ks = [int(NAT[z]) for z in zz]
            for c in range(3):
                for j, k in enumerate(ks):
                    orig[g.coff[c] + b, k] = 5 + j if (b + c) % 2 else -(5 + j)
            ix = np.array([c * 64 + k for k in ks for c in range(3)], np.uint8)
            idx.append(ix)
            cnt[b] = ix.size
        off = np.concatenate([[0], np.cumsum(cnt)])
        idx = np.concatenate(idx)
        blocks = np.arange(g.gn, dtype=np.int32)
        allc = cnt.astype(np.int32)
        out.append(StepCase(family, g, orig, orig.copy(), q1, off, idx, [
            (1, np.zeros(g.gn, np.int32), blocks, allc, True),        # destroys the runs, empties the blocks
            (-1, allc, blocks, allc, True),                           # restores them, coefficient 63 among them
            (1, np.zeros(g.gn, np.int32), blocks, np.minimum(allc, 3), True)]))
    elif family in ("twice", "plain"):
        orig = _random_orig(g, rng)
        cnt = np.full(g.gn, 189, np.int64)
        off = np.concatenate([[0], np.cumsum(cnt)])
        idx = np.concatenate([_all_candidates(g, rng) for _ in range(g.gn)])
        cand = _requant(orig, q, g)
        b1 = rng.permutation(g.gn)[:100].astype(np.int32)
        b2 = rng.permutation(g.gn)[:77].astype(np.int32)
        c1 = rng.integers(1, 60, 100).astype(np.int32)
        c2 = rng.integers(1, 60, 77).astype(np.int32)
        nc1 = np.zeros(g.gn, np.int32)
        nc2 = np.zeros(g.gn, np.int32)
        nc2[b1] = c1
        nc2[b2] = np.maximum(nc2[b2], c2)                             # (restores some of the first call's, and more)
        nc2 = np.minimum(nc2 + 5, 189).astype(np.int32)
        if family == "twice":
            for read_first in (True, False):
                out.append(StepCase(family, g, orig, cand, q, off, idx,
                                    [(1, nc1, b1, c1, read_first), (-1, nc2, b2, c2, True), (1, nc1, b2, c2, True)]))
        else:
            out.append(StepCase(family, g, orig, cand, q, off, idx, [(1, nc1, b1, c1, False), (-1, nc2, b2, c2, False)],
                                with_statistics=False))
    elif family == "420":
        for mask in (1, 6):
            gg = Grid(136, 104, "420", mask)
            orig = _random_orig(gg, rng)
            per = 63 if mask == 1 else 63
            cnt = np.full(gg.gn, per * len(gg.comps), np.int64)
            off = np.concatenate([[0], np.cumsum(cnt)])
            idx = np.concatenate([_all_candidates(gg, rng) for _ in range(gg.gn)])
            cand = _requant(orig, q, gg)
            blocks = rng.permutation(gg.gn).astype(np.int32)
            counts = rng.integers(1, int(cnt[0]) + 1, gg.gn).astype(np.int32)
            nc = np.zeros(gg.gn, np.int32)
            nc[blocks] = counts
            out.append(StepCase(family, gg, orig, cand, q, off, idx,
                                [(1, np.zeros(gg.gn, np.int32), blocks, counts, True), (-1, nc, blocks, counts, True)]))
    else:
        raise KeyError(family)
    return out


# --------------------------------------------------------------------- descent -----
PER_BLOCK = (2.0, 0.2, 0.8)
DESCENT_CNT = 20        # candidates per block of the descent cases' search: an order of one block is worth a descent


def descent_search(g):
    """cnt = DESCENT_CNT everywhere, errors that repeat (ties between blocks, as the product's orders have)."""
    rng = np.random.default_rng(4242 + g.gn)
    cnt = np.full(g.gn, DESCENT_CNT, np.int64)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    err = (rng.integers(0, 4096, int(off[-1])) / 4096.0).astype(F32)
    idx = (np.arange(err.size) % 63 + 1).astype(np.uint8)
    return off, idx, err


def descent_next_cand(g, btc, short):
    """"up": the first btc blocks have candidates left -- all DESCENT_CNT of them, or one (`short`: the order is then
    shorter than per_block * btc for per_block 2.0, the n - 1 cap)."""
    nc = np.full(g.gn, DESCENT_CNT, np.int32)
    nc[:btc] = DESCENT_CNT - 1 if short else 0
    return nc
