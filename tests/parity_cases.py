"""Parity cases shared by the CPU-emulation run (`-m "not gpu"`, tests/test_kernels_emu.py)
and the real-GPU run (`-m gpu`, tests/test_gpu_parity.py): the same kernels, the same
checks, through the same C ABI -- only the library differs."""
import numpy as np

import images
from checkers import assert_bits_equal, oracle

RNG_SEED = 20260921

SIGMAS_BR = [(1.2, 0.0), (7.46953768697, -0.00457628248637), (3.734768843485, -0.271277366628),
             (1.8673844217425, 0.147068973249), (10.6666499623, 0.0),
             (9.24456601467, -0.0724948220913), (2.3770330432, -0.0724948220913),
             (9.04353323561, -0.0724948220913), (1.72547472444, 1.0)]


def case_block_kernels(L, n=1500):
    rng = np.random.default_rng(RNG_SEED)
    blocks = rng.integers(-4096, 4097, size=(n, 64)).astype(np.int16)
    blocks[: n // 2][rng.random((n // 2, 64)) < 0.7] = 0
    blocks = np.concatenate([blocks, np.full((1, 64), 32767, np.int16),
                             np.full((1, 64), -32768, np.int16), np.zeros((2, 64), np.int16)])
    got = L.idct_blocks(blocks)
    exp = np.stack([oracle.idct_block(b) for b in blocks])
    assert_bits_equal(got, exp, "idct blocks")
    px = np.concatenate([rng.integers(-128, 128, size=(n, 64)).astype(np.int16),
                         np.full((1, 64), -128, np.int16), np.full((1, 64), 127, np.int16)])
    got = L.fdct_blocks(px)
    exp = np.stack([oracle.fdct_block(b) for b in px])
    assert_bits_equal(got, exp, "fdct blocks")


def case_dct_double(L, n=1500):
    """dct_double.cc: FP64 block transforms, bit for bit."""
    rng = np.random.default_rng(RNG_SEED + 8)
    blocks = np.concatenate([
        rng.integers(-2048, 2048, size=(n, 64)).astype(np.float64),          # coefficient-like
        rng.random((n // 2, 64)) * 255.0,                                      # pixel-like
        rng.standard_normal((n // 2, 64)) * 10.0 ** rng.integers(-30, 30, (n // 2, 64)),
        np.zeros((1, 64)), -np.zeros((1, 64)), np.full((1, 64), 255.0)])
    for inverse in (False, True):
        got = L.dct_double_blocks(blocks, inverse=inverse)
        exp = np.stack([oracle.dct_double(b, inverse) for b in blocks])
        assert_bits_equal(got, exp, f"dct_double inverse={inverse}")


def case_downsample_component(L, w, h, x0=0, y0=0):
    """ToFloatPixels + SetDownsampledCoefficients (output_image.cc:99-121,265-300), the two
    users of dct_double.cc on the YUV420 path, for the subsampling factors guetzli uses."""
    rgb = images.crop(w, h, x0, y0)
    co = oracle.encode_rgb(rgb)
    for c in range(3):
        px = L.component_to_float_pixels(co[c], w, h)
        assert_bits_equal(px, oracle.to_float_pixels(co[c], w, h), f"ToFloatPixels c={c}")
    for fx, fy in ((2, 2), (1, 1)):
        eu, ev = oracle.downsample_chroma(co, w, h, fx, fy)
        for c, exp in ((1, eu), (2, ev)):
            px = L.component_to_float_pixels(co[c], w, h)
            got = L.component_set_downsampled(px, fx, fy)
            assert_bits_equal(got, exp, f"SetDownsampledCoefficients c={c} {fx}x{fy} {w}x{h}")


def case_encode_quantize_reconstruct(L, w, h, x0=0, y0=0):
    rng = np.random.default_rng(RNG_SEED + w)
    rgb = images.crop(w, h, x0, y0)
    with L.context(rgb, 1.0) as ctx:
        co = ctx.encode_rgb()
        exp = oracle.encode_rgb(rgb)
        assert_bits_equal(co, exp, "encode_rgb")
        q = np.stack([rng.integers(1, 12, size=64), rng.integers(1, 20, size=64),
                      rng.integers(1, 20, size=64)]).astype(np.int32)
        for qq in (None, q):
            cq = ctx.quantize(qq)
            ecq, esrgb, elin = oracle.reconstruct(exp, w, h, qq)
            assert_bits_equal(cq, ecq, "quantize")
            srgb, lin = ctx.reconstruct()
            assert_bits_equal(srgb, esrgb, "reconstruct srgb")
            assert_bits_equal(lin, elin, "reconstruct linear")
        # block updates
        idx = np.unique(np.array([0, ctx.nb - 1, ctx.nb // 2], np.int32))   # must be distinct
        blocks = rng.integers(-300, 300, size=(len(idx), 3, 64)).astype(np.int16)
        ctx.set_coeff_blocks(idx, blocks)
        ecq2 = ecq.copy()
        for i, b in enumerate(idx):
            ecq2[:, b, :] = blocks[i]
        assert_bits_equal(ctx.get_coeffs(), ecq2, "set_coeff_blocks")


def case_blur(L, w, h, configs=SIGMAS_BR):
    rng = np.random.default_rng(RNG_SEED + 7 * w + h)
    plane = (rng.random((h, w)) * 255).astype(np.float32)
    rgb = np.zeros((h, w, 3), np.uint8)
    with L.context(rgb, 1.0) as ctx:
        for s, br in configs:
            got = ctx.probe_blur(plane, s, br)
            exp = oracle.blur(plane, s, br)
            assert_bits_equal(got, exp, f"blur sigma={s} br={br} {w}x{h}")


def _linear_pair(w, h, x0, y0, qscale):
    rgb = images.crop(w, h, x0, y0)
    co = oracle.encode_rgb(rgb)
    q = np.full((3, 64), qscale, np.int32)
    cq, _, lin1 = oracle.reconstruct(co, w, h, q)
    lut = oracle.srgb_table()
    lin0 = lut[rgb].astype(np.float32).transpose(2, 0, 1).copy()
    return rgb, co, cq, lin0, lin1


def case_stages(L, w, h, x0=40, y0=60, qscale=6):
    """opsin -> separate_frequencies -> mask -> diffmap, each against the oracle."""
    rgb, co, cq, lin0, lin1 = _linear_pair(w, h, x0, y0, qscale)
    with L.context(rgb, 1.0) as ctx:
        x0_, x1_ = oracle.opsin(lin0), oracle.opsin(lin1)
        assert_bits_equal(ctx.probe_opsin(lin0), x0_, "opsin(orig)")
        assert_bits_equal(ctx.probe_opsin(lin1), x1_, "opsin(cand)")
        for xyb in (x0_, x1_):
            got = ctx.probe_separate_frequencies(xyb)
            exp = oracle.separate_frequencies(xyb)
            names = ["lf0", "lf1", "lf2", "mf0", "mf1", "mf2", "hf0", "hf1", "uhf0", "uhf1"]
            for i, nm in enumerate(names):
                if nm == "mf2":
                    continue   # dead plane in the reference (wmul[5] == 0), never computed
                assert_bits_equal(got[i], exp[i], f"separate_frequencies {nm}")
        for a, b in ((x0_, x1_), (x0_, x0_)):
            gm, gdc = ctx.probe_mask(a, b)
            em, edc = oracle.mask(a, b)
            assert_bits_equal(gm, em, "mask")
            assert_bits_equal(gdc, edc, "mask_dc")
        gd, gs = ctx.probe_diffmap(lin0, lin1)
        ed, es = oracle.diffmap(lin0, lin1)
        assert_bits_equal(gd, ed, "diffmap")
        assert gs == np.float32(es)


def case_compare(L, w, h, x0=0, y0=0, qscales=(1, 3, 9), target=0.971769):
    """The drop-in call sequence of TryQuantMatrix: encode -> quantize(q) -> compare."""
    rgb = images.crop(w, h, x0, y0) if max(w, h) <= 444 else images.tiled(w, h)
    oc = oracle.comparator(rgb, target)
    with L.context(rgb, target) as ctx:
        co = ctx.encode_rgb()
        assert_bits_equal(co, oracle.encode_rgb(rgb), "encode_rgb")
        for qs in qscales:
            q = np.full((3, 64), qs, np.int32)
            cq = ctx.quantize(q)
            dist, dm, bm = ctx.compare()
            edist, edm = oc.compare(cq)
            assert_bits_equal(dm, edm, f"distmap q={qs}")
            assert dist == edist
            # block maxima + weights
            pad = np.zeros((ctx.bh * 8, ctx.bw * 8), np.float32)
            pad[:h, :w] = edm
            ebm = pad.reshape(ctx.bh, 8, ctx.bw, 8).max(axis=(1, 3)).reshape(-1)
            assert_bits_equal(bm, ebm, "block max")
            for direction in (1, -1):
                for r in (1, 3):
                    assert_bits_equal(ctx.block_weights(direction, r, 1.0),
                                      oc.block_weights(direction, r, 1.0, edm),
                                      "block weights")
    oc.close()


def case_block_search(L, w, h, x0=300, y0=150, qs=3, target=0.971769):
    """Phase A of SelectFrequencyMasking through gz_block_zeroing_orders."""
    rgb = images.crop(w, h, x0, y0) if max(w, h) <= 444 else images.tiled(w, h)
    oc = oracle.comparator(rgb, target)
    with L.context(rgb, target) as ctx:
        co = ctx.encode_rgb()
        cq = ctx.quantize(np.full((3, 64), qs, np.int32))
        off, idx, err = ctx.block_zeroing_orders()
        eoff, eidx, eerr = oc.block_zeroing_orders(cq, co)
        assert_bits_equal(off, eoff, "candidate offsets")
        assert_bits_equal(idx, eidx, "candidate coefficient indices")
        assert_bits_equal(err, eerr, "candidate errors")
        assert off[-1] > 0
    oc.close()


def case_global_order(L, w, h, x0=300, y0=150, qs=3, target=0.971769, census=None):
    """Phase B's global candidate order on the device (processor.cc:622-663): the construction
    from the reference's definition, the device-side block weights
    (ComputeBlockErrorAdjustmentWeights, pinned through the oracle) and max_block_error
    bookkeeping, and single-coefficient edits.  The restatements of tests/order_domain.py are pinned
    here on the way: on these arrays they give what the oracle and the loops below give (census: the
    arms this photograph takes, counted by them)."""
    import order_domain as od
    g = od.Grid(w, h)
    rng = np.random.default_rng(RNG_SEED + 3 * w + h)
    rgb = images.crop(w, h, x0, y0) if max(w, h) <= 444 else images.tiled(w, h)
    oc = oracle.comparator(rgb, target)
    with L.context(rgb, target) as ctx:
        ctx.encode_rgb()
        cq = ctx.quantize(np.full((3, 64), qs, np.int32))
        off, idx, err = ctx.block_zeroing_orders()
        dist, dm, bmax = ctx.compare()
        nb = ctx.nb
        cnt = np.diff(off)
        max_err = np.zeros(nb, np.float32)
        ctx.order_reset()
        for direction, use_dm in ((1, False), (1, True), (-1, True), (-1, True)):
            next_cand = (rng.integers(0, 1000, nb) % (cnt + 1)).astype(np.int32)
            for radius in (1, 2, 4):
                zero = np.zeros_like(dm)
                wgt = oc.block_weights(direction, radius, 1.0, dm if use_dm else zero)
                assert_bits_equal(od.weights_of(g, bmax, target, direction, radius, 1.0, use_dm, census), wgt,
                                  "order_domain.weights_of")
                # the reference's construction loop
                exp = []
                btc = 0
                for b in range(nb):
                    if wgt[b] == 0:
                        continue
                    e = err[off[b]:off[b + 1]]
                    at = next_cand[b]
                    if direction > 0:
                        vals = (e[at:] - max_err[b]) / wgt[b]
                        btc += at < cnt[b]
                    else:
                        vals = (max_err[b] - e[:at][::-1]) / wgt[b]
                        btc += at > 0
                    exp.extend((b, v) for v in vals.astype(np.float32))
                limit = np.float32(0.75) * np.float32(target)
                mb, mv, mbtc, mbelow = od.build_order(off, err, next_cand, max_err, wgt, direction, float(limit), census)
                assert mbtc == btc and mb.tolist() == [b for b, _ in exp], "order_domain.build_order"
                assert_bits_equal(mv, np.array([v for _, v in exp], np.float32), "order_domain.build_order")
                total, got_btc, below = ctx.order_build_auto(direction, radius, 1.0, use_dm,
                                                             next_cand, limit=float(limit))
                assert total == len(exp) and got_btc == btc and below == mbelow, (total, len(exp), got_btc, btc)
                got = ctx.order_fetch(0, total)
                if total:
                    eb = np.array([b for b, _ in exp], np.int32)
                    ev = np.array([v for _, v in exp], np.float32)
                    assert_bits_equal(got["block"], eb, "order blocks")
                    assert_bits_equal(got["val"], ev, "order vals")
                    assert below == int((ev < limit).sum())
                # the two-halves form (construction enqueued ahead of the wait) = the one-call form
                ctx.order_build_auto_begin(direction, radius, 1.0, use_dm, next_cand, limit=float(limit))
                assert ctx.order_build_auto_end() == (total, btc, below)
                assert_bits_equal(ctx.order_fetch(0, total), got, "order after _begin/_end")
                # explicit-weights entry point gives the same order
                t2, b2, _ = ctx.order_build(direction, next_cand, max_err, wgt)
                assert (t2, b2) == (total, btc)
                assert_bits_equal(ctx.order_fetch(0, t2), got, "gz_order_build vs _auto")
            # leave the last radius' weights in place and advance, as the driver does
            thr = np.float32(rng.random() * 0.3)
            ctx.order_build_auto(direction, 4, 1.0, use_dm, next_cand)
            ctx.order_advance(float(thr), direction)
            wgt = oc.block_weights(direction, 4, 1.0, dm if use_dm else np.zeros_like(dm))
            assert_bits_equal(od.advance(max_err, wgt, thr, direction),
                              (max_err + (wgt * thr) * np.float32(direction)).astype(np.float32), "order_domain.advance")
            max_err = (max_err + (wgt * thr) * np.float32(direction)).astype(np.float32)
        # whole-block steps (processor.cc:704-736): zero / restore the next candidates
        def quantize(raw, q):
            r = int(np.fmod(raw, q))
            d = q - r if 2 * r > q else (-q - r if -2 * r > q else -r)
            return np.int16(raw + d)
        co = ctx.get_coeffs()
        orig = ctx.encode_rgb()
        for direction in (1, -1):
            exp = co.copy()
            if direction > 0:
                next_cand = (rng.integers(0, 1000, nb) % (cnt + 1)).astype(np.int32)
                counts = (rng.integers(0, 1000, nb) % (cnt - next_cand + 1)).astype(np.int32)
            else:
                next_cand = (rng.integers(0, 1000, nb) % (cnt + 1)).astype(np.int32)
                counts = (rng.integers(0, 1000, nb) % (next_cand + 1)).astype(np.int32)
            sel = np.flatnonzero(counts > 0).astype(np.int32)
            for b in sel:
                for j in range(counts[b]):
                    p = next_cand[b] + j if direction > 0 else next_cand[b] - 1 - j
                    ix = int(idx[off[b] + p])
                    c, k = ix // 64, ix % 64
                    ob = orig[c, b].astype(np.int64)
                    newval = 0 if direction > 0 else int(quantize(int(ob[k]), qs))
                    precious = False
                    if newval == 0 and k in (1, 8):
                        hf = sum(abs(int(ob[i])) for i in range(3, 64) if not ((i & 7) < 3 and i < 24))
                        precious = abs(int(ob[k])) >= (4 if hf < 60 else 8)
                    if not precious:
                        exp[c, b, k] = newval
            qs_all = np.full((3, 64), qs, np.int32)
            assert_bits_equal(od.apply_steps(g, co, orig, qs_all, off, idx, next_cand, direction, sel, counts[sel],
                                             census).reshape(exp.shape), exp, "order_domain.apply_steps")
            assert_bits_equal(od.hist_delta(g, co, exp, qs_all, census), od.ac_hist(g, exp, qs_all) - od.ac_hist(g, co, qs_all),
                              "order_domain.hist_delta")
            exp_delta = od.hist_delta(g, co, exp, qs_all)
            ctx.order_build_auto(direction, 1, 1.0, True, next_cand)   # uploads next_cand
            before = ctx.jpeg_histograms(qs_all)                        # also: the symbols' quantiser
            ctx.apply_candidate_steps(direction, sel, counts[sel])
            delta = ctx.steps_histogram_delta()
            co = ctx.get_coeffs()
            assert_bits_equal(co, exp, f"apply_candidate_steps direction {direction}")
            # the statistics change the steps report == a recount of the whole image
            after = ctx.jpeg_histograms(qs_all)
            assert_bits_equal(delta, after[1].astype(np.int64) - before[1].astype(np.int64),
                              f"steps_histogram_delta direction {direction}")
            assert_bits_equal(delta, exp_delta, f"steps_histogram_delta == order_domain.hist_delta, direction {direction}")
        cq = co
        # single-coefficient edits == block scatter
        pos = rng.choice(3 * nb * 64, size=min(500, nb), replace=False).astype(np.int32)
        val = rng.integers(-50, 50, pos.size).astype(np.int16)
        ctx.apply_coeff_edits(pos, val)
        expc = cq.copy().reshape(-1)
        expc[pos] = val
        assert_bits_equal(ctx.get_coeffs().reshape(-1), expc, "apply_coeff_edits")
    oc.close()


def case_patched_candidate_planes(L, w, h, x0=0, y0=0, qs=3, target=0.971769, rounds=3, expect_ahead=True):
    """gz_config.patch_reconstruct through the C ABI alone: after bulk steps on a minority of the block positions
    (gz_apply_candidate_steps) and single-coefficient edits elsewhere (gz_apply_coeff_edits), a Compare that relies on
    the patched linear planes (and, in mode 2, checks them against a full reconstruction itself) gives the distance,
    distance map and per-block maxima, bit for bit, of the same coefficients put in place as a whole (gz_set_coeffs:
    full reconstruction).  Ragged sizes patch partial blocks at the right / bottom edge.  A change of more than half
    of the positions, or a whole-image writer in between, drops the patches' claim."""
    rng = np.random.default_rng(RNG_SEED + 5 * w + h)
    rgb = images.crop(w, h, x0, y0) if max(w, h) <= 444 else images.tiled(w, h)
    q = np.full((3, 64), qs, np.int32)
    with L.context(rgb, target) as ctx:
        cfg = ctx.set_config(patch_reconstruct=2)
        expect_ahead = expect_ahead and cfg.opsin_ahead != 0 and cfg.single_stream != 1   # (the suite's forced modes)
        ctx.encode_rgb()
        ctx.quantize(q)
        off, idx, err = ctx.block_zeroing_orders()
        nb = ctx.nb
        cnt = np.diff(off)
        ctx.order_reset()
        ctx.compare()                                    # the full reconstruction: the planes are the candidate's
        next_cand = np.zeros(nb, np.int32)
        for r in range(rounds):
            ctx.order_build_auto(1, 1, 1.0, True, next_cand)     # (uploads next_cand)
            ctx.jpeg_histograms(q)                               # (the steps' statistics path)
            some = rng.random(nb) < (0.3 if r < rounds - 1 else 0.8)
            counts = np.where(some, np.minimum(cnt - next_cand, 1 + rng.integers(0, 3, nb)), 0).astype(np.int32)
            sel = np.flatnonzero(counts > 0).astype(np.int32)
            before = L.compare_counters(all=True)
            ctx.apply_candidate_steps(1, sel, counts[sel])
            ctx.steps_histogram_delta()
            next_cand = next_cand + counts
            pos = rng.choice(3 * nb * 64, size=min(40, nb // 4), replace=False).astype(np.int32)   # (fewer than half of the positions)
            ctx.apply_coeff_edits(pos, rng.integers(-40, 40, pos.size).astype(np.int16))
            got = ctx.compare()
            patched, checked, compares, ahead, ahead_checked = (a - b for a, b in zip(L.compare_counters(all=True), before))
            # (the last round touches most positions: no patches, the Compare reconstructs)
            assert (patched, checked, compares) == ((1, 1, 1) if 2 * sel.size <= nb else (0, 0, 1)), (patched, checked, sel.size, nb)
            # (the opsin image kept ahead as well -- gz_config.opsin_ahead, a context alone on its device -- and checked)
            assert ahead == ahead_checked and ahead in ((0, 1) if patched else (0,))
            if patched and expect_ahead:
                assert ahead == 1
            co = ctx.get_coeffs()
            ctx.set_coeffs(co)
            before = L.compare_counters()
            exp = ctx.compare()
            assert L.compare_counters()[0] == before[0]
            for g, e, what in zip(got, exp, ("distance", "distance map", "block maxima")):
                assert_bits_equal(np.asarray(g, np.float32), np.asarray(e, np.float32), f"patched {what}, round {r}")


ZIGZAG_NATURAL = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
                  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                  35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                  58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def expected_jpeg_histograms(cq, q):
    """BuildDCHistograms / BuildACHistograms (jpeg_data_writer.cc:241-275) from their
    definition, on quantised values cq / q (C truncation)."""
    cq = cq.astype(np.int64)
    qq = np.asarray(q, np.int64)[:, None, :]
    qv = np.sign(cq) * (np.abs(cq) // qq)
    counts = np.zeros((2, 3, 256), np.int64)
    for c in range(3):
        dc = qv[c, :, 0]
        diff = np.abs(np.diff(np.concatenate([[0], dc])))
        nbits = np.where(diff > 0, np.floor(np.log2(np.maximum(diff, 1))).astype(np.int64) + 1, 0)
        np.add.at(counts[0, c], nbits, 1)
        zz = qv[c][:, ZIGZAG_NATURAL]
        for blk in zz:
            run = 0
            for k in range(1, 64):
                v = int(blk[k])
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    counts[1, c, 0xf0] += 1
                    run -= 16
                counts[1, c, (run << 4) + abs(v).bit_length()] += 1
                run = 0
            if run > 0:
                counts[1, c, 0] += 1
    return counts.astype(np.uint32)


def jpeg_entropy_inputs(w, h, x0=0, y0=0):
    """The inputs of case_jpeg_entropy: (rgb, original coefficients, [(dequantised coefficients, q or None, is_grey)],
    the wild case's array)."""
    rng = np.random.default_rng(RNG_SEED + 31 * w + h)
    rgb = images.crop(w, h, x0, y0) if max(w, h) <= 444 else images.tiled(w, h)
    co = oracle.encode_rgb(rgb)
    nb = co.shape[1]
    qs = [None,
          np.full((3, 64), 3, np.int32),
          np.stack([rng.integers(1, 9, 64), rng.integers(1, 30, 64), rng.integers(1, 30, 64)]).astype(np.int32),
          np.stack([rng.integers(200, 400, 64), rng.integers(1, 30, 64), rng.integers(1, 30, 64)]).astype(np.int32)]
    cases = []
    for q in qs:
        cq, _, _ = oracle.reconstruct(co, w, h, q)
        cases.append((cq, q, False))
    # dense large-magnitude coefficients (long MCUs, long codes, ZRL runs), q = 1
    wild = rng.integers(-2040, 2041, size=co.shape).astype(np.int16)
    wild[:, :, 1:][rng.random((3, nb, 63)) < 0.35] = 0
    wild[:, nb // 3:nb // 3 + 2, 1:40] = 0
    cases.append((wild, np.ones((3, 64), np.int32), False))
    # grey image: both chroma planes zero -> a single-component frame
    grey = cases[1][0].copy()
    grey[1:] = 0
    cases.append((grey, qs[1], True))
    return rgb, co, cases, wild


def case_jpeg_entropy(L, host, w, h, x0=0, y0=0, check_histograms=True):
    """Device symbol statistics + device scan (gz_jpeg_histograms / gz_jpeg_scan) with the
    host-built marker segments must reproduce the reference's WriteJpeg byte for byte."""
    from checkers import ref
    rgb, co, cases, wild = jpeg_entropy_inputs(w, h, x0, y0)
    with L.context(rgb, 1.0) as ctx:
        for cq, q, is_grey in cases:
            qq = np.ones((3, 64), np.int32) if q is None else q
            ctx.set_coeffs(cq)
            counts = ctx.jpeg_histograms(qq)
            if check_histograms:
                assert_bits_equal(counts, expected_jpeg_histograms(cq, qq), "jpeg histograms")
            ncomp = 1 if is_grey else 3
            head, depth, code = host.jpeg_head(counts, w, h, q, ncomp)
            n = ctx.jpeg_scan(ncomp, depth, code)
            scan = ctx.jpeg_scan_bytes()
            assert len(scan) == n
            # the scan's length in bits is a function of the symbol statistics and the code lengths
            # alone (what the search driver bounds a candidate's size with, without coding it);
            # the stuffed bytes are the 0xFF bytes of the stream
            bits, stuffed = ctx.jpeg_scan_bits()
            cnt = np.asarray(counts, np.int64)[:, :ncomp]
            extra = np.arange(256) & 15
            assert bits == int((cnt * (depth[:, :ncomp].astype(np.int64) + extra)).sum())
            assert n == (bits + 7) // 8 + stuffed and stuffed == scan.count(b"\xff\x00")
            got = head + scan + b"\xff\xd9"
            exp = host.write_jpeg(cq, w, h, q)           # pinned to the reference in
            assert got == exp, (len(got), len(exp))      # test_host_encoder.test_write_jpeg_bytes
            if ref is not None and q is not None and not is_grey and cq is not wild:
                assert got == ref.write_jpeg(co, w, h, q)
            ctx.jpeg_scan_keep()
            assert ctx.jpeg_scan_bytes(kept=True) == scan


# ------------------------------------------------------------------ YUV 4:2:0 (row f4) --
def colourful(w, h):
    """Saturated reds / blues over dark and bright backgrounds with soft and hard edges: makes
    every branch of PreProcessChannel (sharpen map, blur map, neither) non-trivial."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    r = 60 + 150 * (np.sin(x / 9.0) > 0) * (y < 0.6 * h) + 40 * np.sin(y / 7.0)
    g = 40 + 30 * np.cos((x + y) / 13.0) + 120 * (x > 0.7 * w)
    b = 50 + 160 * (np.cos(y / 11.0) > 0.3) * (x < 0.5 * w) + 100 * (x > 0.7 * w)
    m = ((x - 0.5 * w) ** 2 + (y - 0.5 * h) ** 2) < (0.2 * min(w, h)) ** 2
    r[m], g[m], b[m] = 220, 30, 40
    return np.ascontiguousarray(np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8))


def case_frame420(L, w, h, chk, x0=0, y0=0, rgb=None):
    """gz_downsample (OutputImage::Downsample + PreProcessChannel), the 4:2:0 pixel model
    (gz_reconstruct), gz_compare and gz_block_weights_factor on a 4:2:0 frame against `chk`."""
    rng = np.random.default_rng(RNG_SEED + 11 * w + h)
    if rgb is None:
        rgb = images.crop(w, h, x0, y0)
    co = chk.encode_rgb(rgb)
    exp = chk.downsample(co, w, h)
    oc = chk.comparator(rgb, 1.0)
    with L.context(rgb, 1.0) as ctx:
        ctx.encode_rgb()
        got = ctx.downsample()
        assert ctx.frame_layout() == (2, ctx.nb, ctx.nbc)
        assert_bits_equal(got, exp, f"downsample {w}x{h}")
        q = np.stack([rng.integers(1, 8, 64), rng.integers(1, 12, 64),
                      rng.integers(1, 12, 64)]).astype(np.int32)
        for qq in (None, q):
            cq = ctx.quantize(qq)
            ecq, esrgb, elin = chk.reconstruct420(exp, w, h, qq, shuffle=7)
            assert_bits_equal(cq, ecq, "quantize (4:2:0)")
            srgb, lin = ctx.reconstruct()
            assert_bits_equal(srgb, esrgb, "reconstruct srgb (4:2:0)")
            assert_bits_equal(lin, elin, "reconstruct linear (4:2:0)")
        dist, dm, _ = ctx.compare()
        edist, edm = oc.compare420(cq)
        assert_bits_equal(dm, edm, "distance map (4:2:0)")
        assert dist == edist
        for direction in (1, -1):
            for factor in (1, 2):
                for radius in (1, 3):
                    gotw = ctx.block_weights_factor(direction, radius, 0.97, factor)
                    expw = oc.block_weights_factor(direction, radius, 0.97, factor, edm)
                    assert_bits_equal(gotw, expw, f"block weights factor {factor} dir {direction}")
        # back to 4:4:4
        ctx.encode_rgb()
        assert ctx.frame_layout()[0] == 1
    oc.close()


def case_block_search420(L, w, h, chk, x0=0, y0=0, qs=3, lookahead=3, new_model=True):
    """Phase A on a 4:2:0 frame: luma candidates on the 8x8 grid (mask 1), chroma candidates on
    the 16x16 grid with the 2x2 pixel model and the maximum over the sub-blocks (mask 6)."""
    rgb = images.crop(w, h, x0, y0)
    co = chk.encode_rgb(rgb)
    orig = chk.downsample(co, w, h)
    oc = chk.comparator(rgb, 0.971769)
    with L.context(rgb, 0.971769) as ctx:
        ctx.encode_rgb()
        ctx.downsample(download=False)
        cq = ctx.quantize(np.full((3, 64), qs, np.int32))
        for mask in (1, 6):
            off, idx, err = ctx.block_zeroing_orders(lookahead, new_model, comp_mask=mask)
            eoff, eidx, eerr = oc.block_zeroing_orders_masked(cq, orig, True, mask, lookahead, new_model)
            assert_bits_equal(off, eoff, f"offsets mask {mask}")
            assert_bits_equal(idx, eidx, f"candidates mask {mask}")
            assert_bits_equal(err, eerr, f"errors mask {mask}")
    oc.close()


def case_block_search_masks444(L, w, h, chk, x0=0, y0=0, qs=3, lookahead=3, new_model=True):
    """Component masks and non-default Params on a 4:4:4 frame."""
    rgb = images.crop(w, h, x0, y0)
    orig = chk.encode_rgb(rgb)
    oc = chk.comparator(rgb, 0.971769)
    with L.context(rgb, 0.971769) as ctx:
        ctx.encode_rgb()
        cq = ctx.quantize(np.full((3, 64), qs, np.int32))
        for mask in (7, 1, 6):
            off, idx, err = ctx.block_zeroing_orders(lookahead, new_model, comp_mask=mask)
            eoff, eidx, eerr = oc.block_zeroing_orders_masked(cq, orig, False, mask, lookahead, new_model)
            assert_bits_equal(off, eoff, f"offsets mask {mask}")
            assert_bits_equal(idx, eidx, f"candidates mask {mask}")
            assert_bits_equal(err, eerr, f"errors mask {mask}")
    oc.close()


def jpeg_entropy420_quants(w, h):
    """The quantisers of case_jpeg_entropy420."""
    rng = np.random.default_rng(RNG_SEED + 5 * w + h)
    return [np.full((3, 64), 2, np.int32),
            np.stack([rng.integers(1, 9, 64), rng.integers(1, 30, 64), rng.integers(1, 30, 64)]).astype(np.int32),
            np.stack([np.full(64, 3), np.full(64, 4000), np.full(64, 4000)]).astype(np.int32)]   # chroma -> all zero


def case_jpeg_entropy420(L, H, w, h, chk, x0=0, y0=0):
    """The device entropy coder on a 4:2:0 frame (MCUs of 2x2 luma + Cb + Cr blocks, padding
    blocks, DC prediction in scan order) + the host head == the reference's WriteJpeg."""
    rgb = images.crop(w, h, x0, y0)
    co = chk.encode_rgb(rgb)
    orig = chk.downsample(co, w, h)
    with L.context(rgb, 1.0) as ctx:
        ctx.encode_rgb()
        ctx.downsample(download=False)
        qs = jpeg_entropy420_quants(w, h)
        for q in qs:
            cq = ctx.quantize(q)
            exp = chk.write_jpeg420(orig, w, h, q)
            assert H.write_jpeg(cq, w, h, q, factor=2) == exp, "host writer (4:2:0)"
            y, cb, cr = ctx.split420(cq)
            ncomp = 3 if (cb.any() or cr.any()) else 1
            counts = ctx.jpeg_histograms(q, ncomp)
            head, depth, code = H.jpeg_head(counts, w, h, q, ncomp=ncomp, factor=2)
            n = ctx.jpeg_scan(ncomp, depth, code)
            scan = ctx.jpeg_scan_bytes()
            assert len(scan) == n
            # the scan's length in bits is a function of the symbol statistics and the code lengths
            # alone (what the search driver bounds a candidate's size with, without coding it);
            # the stuffed bytes are the 0xFF bytes of the stream
            bits, stuffed = ctx.jpeg_scan_bits()
            cnt = np.asarray(counts, np.int64)[:, :ncomp]
            extra = np.arange(256) & 15
            assert bits == int((cnt * (depth[:, :ncomp].astype(np.int64) + extra)).sum())
            assert n == (bits + 7) // 8 + stuffed and stuffed == scan.count(b"\xff\x00")
            got = head + scan + b"\xff\xd9"
            assert got == exp, (len(got), len(exp), ncomp)


def case_global_order420(L, w, h, chk, x0=0, y0=0, qs=3, target=0.971769, census=None):
    """Phase B's order on the chroma grid of a 4:2:0 frame: device-side weights over 16x16
    areas, the construction loop, whole-block steps on components 1 and 2 with their
    statistics change.  (order_domain's restatements pinned on the way, as in case_global_order.)"""
    import order_domain as od
    g = od.Grid(w, h, "420", 6)
    rng = np.random.default_rng(RNG_SEED + 13 * w + h)
    rgb = images.crop(w, h, x0, y0)
    oc = chk.comparator(rgb, target)
    with L.context(rgb, target) as ctx:
        ctx.encode_rgb()
        orig = ctx.downsample()
        q = np.full((3, 64), qs, np.int32)
        cq = ctx.quantize(q)
        off, idx, err = ctx.block_zeroing_orders(comp_mask=6)
        dist, dm, bmax = ctx.compare()
        gn = ctx.nbc
        cnt = np.diff(off)
        max_err = np.zeros(gn, np.float32)
        ctx.order_reset()
        for direction in (1, -1):
            next_cand = (rng.integers(0, 1000, gn) % (cnt + 1)).astype(np.int32)
            for radius in (1, 2):
                wgt = oc.block_weights_factor(direction, radius, 1.0, 2, dm)
                assert_bits_equal(od.weights_of(g, bmax, target, direction, radius, 1.0, True, census), wgt,
                                  "order_domain.weights_of (factor 2)")
                exp = []
                btc = 0
                for b in range(gn):
                    if wgt[b] == 0:
                        continue
                    e = err[off[b]:off[b + 1]]
                    at = next_cand[b]
                    if direction > 0:
                        vals = (e[at:] - max_err[b]) / wgt[b]
                        btc += at < cnt[b]
                    else:
                        vals = (max_err[b] - e[:at][::-1]) / wgt[b]
                        btc += at > 0
                    exp.extend((b, v) for v in vals.astype(np.float32))
                mb, mv, mbtc, _ = od.build_order(off, err, next_cand, max_err, wgt, direction, None, census)
                assert mbtc == btc and mb.tolist() == [b for b, _ in exp], "order_domain.build_order"
                assert_bits_equal(mv, np.array([v for _, v in exp], np.float32), "order_domain.build_order")
                total, got_btc, _ = ctx.order_build_auto(direction, radius, 1.0, True, next_cand)
                assert total == len(exp) and got_btc == btc, (total, len(exp), got_btc, btc)
                got = ctx.order_fetch(0, total)
                if total:
                    assert_bits_equal(got["block"], np.array([b for b, _ in exp], np.int32), "order blocks")
                    assert_bits_equal(got["val"], np.array([v for _, v in exp], np.float32), "order vals")
        # whole-block steps
        def quantize(raw, qq):
            r = int(np.fmod(raw, qq))
            d = qq - r if 2 * r > qq else (-qq - r if -2 * r > qq else -r)
            return np.int16(raw + d)
        co = ctx.get_coeffs()
        coff = [0, ctx.nb, ctx.nb + ctx.nbc]
        for direction in (1, -1):
            exp = co.copy()
            next_cand = (rng.integers(0, 1000, gn) % (cnt + 1)).astype(np.int32)
            if direction > 0:
                counts = (rng.integers(0, 1000, gn) % (cnt - next_cand + 1)).astype(np.int32)
            else:
                counts = (rng.integers(0, 1000, gn) % (next_cand + 1)).astype(np.int32)
            sel = np.flatnonzero(counts > 0).astype(np.int32)
            for b in sel:
                for j in range(counts[b]):
                    p = next_cand[b] + j if direction > 0 else next_cand[b] - 1 - j
                    ix = int(idx[off[b] + p])
                    c, k = ix // 64, ix % 64
                    ob = orig[coff[c] + b].astype(np.int64)
                    newval = 0 if direction > 0 else int(quantize(int(ob[k]), qs))
                    precious = False
                    if newval == 0 and k in (1, 8):
                        hf = sum(abs(int(ob[i])) for i in range(3, 64) if not ((i & 7) < 3 and i < 24))
                        precious = abs(int(ob[k])) >= (4 if hf < 60 else 8)
                    if not precious:
                        exp[coff[c] + b, k] = newval
            assert_bits_equal(od.apply_steps(g, co, orig, q, off, idx, next_cand, direction, sel, counts[sel], census), exp,
                              "order_domain.apply_steps (4:2:0)")
            exp_delta = od.hist_delta(g, co, exp, q, census)
            assert_bits_equal(exp_delta, od.ac_hist(g, exp, q) - od.ac_hist(g, co, q), "order_domain.hist_delta (4:2:0)")
            ctx.order_build_auto(direction, 1, 1.0, True, next_cand)
            before = ctx.jpeg_histograms(q)
            ctx.apply_candidate_steps(direction, sel, counts[sel])
            delta = ctx.steps_histogram_delta()
            co = ctx.get_coeffs()
            assert_bits_equal(co, exp, f"apply_candidate_steps (4:2:0) direction {direction}")
            after = ctx.jpeg_histograms(q)
            assert_bits_equal(delta, after[1].astype(np.int64) - before[1].astype(np.int64),
                              f"steps_histogram_delta (4:2:0) direction {direction}")
            assert_bits_equal(delta, exp_delta, f"steps_histogram_delta == order_domain.hist_delta (4:2:0), direction {direction}")
    oc.close()


def case_compare_blocks(L, w, h, x0=0, y0=0, qs=3, n=24, case=None, expect_zero=False):
    """gz_compare_blocks == Comparator::SwitchBlock + CompareBlock (the per-block seam).  With `case` (a
    fields.SearchCase) the image, the target and the candidate coefficients are the case's, not the photograph's and
    its quantised copy, and every block of the bottom row and of the right column is evaluated as well."""
    rng = np.random.default_rng(RNG_SEED + 17 * w + h)
    rgb = images.crop(w, h, x0, y0) if case is None else case.rgb
    target = 0.971769 if case is None else case.target
    oc = oracle.comparator(rgb, target)
    with L.context(rgb, target) as ctx:
        ctx.encode_rgb()
        if case is None:
            cq = ctx.quantize(np.full((3, 64), qs, np.int32))
        else:
            cq = np.ascontiguousarray(case.cand, np.int16)
            ctx.set_coeffs(cq)
        bw = ctx.bw
        xy, blocks, exp = [], [], []
        for _ in range(n):
            b = int(rng.integers(0, ctx.nb))
            cand = cq.copy()
            for _ in range(int(rng.integers(0, 4))):   # zero a few coefficients of the block
                cand[int(rng.integers(0, 3)), b, int(rng.integers(1, 64))] = 0
            if case is not None and len(xy) % 3:       # ... or, as the search does on its way, about half or all
                gone = rng.random((3, 64)) < (0.5, 1.0)[len(xy) % 3 - 1]
                gone[:, 0] = False
                cand[:, b, :][gone] = 0
            xy.append((b % bw, b // bw))
            blocks.append(cand[:, b, :])
            exp.append(oc.compare_block(cand, b % bw, b // bw))
        if case is not None:   # the ragged edges: the bottom row and the right column, as they stand
            edge = [(bx, ctx.bh - 1) for bx in range(bw)] + [(bw - 1, by) for by in range(ctx.bh - 1)]
            for bx, by in edge:
                xy.append((bx, by))
                blocks.append(cq[:, by * bw + bx, :])
                exp.append(oc.compare_block(cq, bx, by))
        what = "" if case is None else f" of {case.name}"
        got = ctx.compare_blocks(np.array(xy), np.stack(blocks))
        assert_bits_equal(got, np.array(exp, np.float64), "CompareBlock" + what)
        if expect_zero:
            assert (np.array(exp) == 0.0).any(), f"no block error{what} is exactly 0.0"
        # the pixel form of the seam (gz_compare_block_pixels): the windows' YCbCr pixels are the
        # integer IDCT of their blocks, edge-replicated as OutputImageComponent::ToPixels does
        px = L.idct_blocks(np.stack(blocks).reshape(-1, 64)).reshape(-1, 3, 8, 8)
        for i, (bx, by) in enumerate(xy):
            vw, vh = min(8, w - 8 * bx), min(8, h - 8 * by)
            px[i, :, :, vw:] = px[i, :, :, vw - 1:vw]
            px[i, :, vh:, :] = px[i, :, vh - 1:vh, :]
        got_px = ctx.compare_block_pixels(np.array(xy), px.reshape(-1, 3, 64))
        assert_bits_equal(got_px, np.array(exp, np.float64), "CompareBlock (pixels)" + what)
    oc.close()


# --------------------------------------------- phase A on the search cases (tests/fields.py) --
_search_expected = {}


def search_expected(case, w, h, frame420=False):
    """The oracle's (offsets, indices, errors, census) of one fields.SearchCase: computed once per process and
    shared by the tests that need it (callers leave the arrays unchanged)."""
    key = (case.name, w, h, frame420)
    if key not in _search_expected:
        oc = oracle.comparator(case.rgb, case.target)
        oracle.census_reset()
        if frame420 or case.comp_mask != 7:
            r = oc.block_zeroing_orders_masked(case.cand, case.orig, frame420, case.comp_mask, case.lookahead,
                                               case.new_model)
        else:
            r = oc.block_zeroing_orders(case.cand, case.orig, case.lookahead, case.new_model)
        census = oracle.search_census()
        oc.close()
        for a in r:
            a.setflags(write=False)
        _search_expected[key] = r + (census,)
    return _search_expected[key]


def _check_search(ctx, case, w, h, frame420):
    off, idx, err = ctx.block_zeroing_orders(case.lookahead, case.new_model, comp_mask=case.comp_mask)
    eoff, eidx, eerr, census = search_expected(case, w, h, frame420)
    assert_bits_equal(off, eoff, f"candidate offsets of {case.name}")
    assert_bits_equal(idx, eidx, f"candidate coefficient indices of {case.name}")
    assert_bits_equal(err, eerr, f"candidate errors of {case.name}")
    assert ctx.search_evaluations() == census["search_evaluations"], case.name


def case_search_domain(L, w, h, only=None):
    """gz_block_zeroing_orders[_masked] on every search case of a 4:4:4 frame (tests/fields.py: search_cases)
    against the oracle, bit for bit: offsets, candidate indices, errors; and gz_search_evaluations against the number
    of CompareBlock calls the oracle's search loops made.  The original coefficients are the image's own
    (gz_encode_rgb) or, where the case says so, foreign ones (gz_set_orig_coeffs: the JPEG-input path)."""
    import fields
    n = 0
    for case in fields.search_cases(w, h, only):
        with L.context(case.rgb, case.target) as ctx:
            co = ctx.encode_rgb()
            if case.foreign:
                ctx.set_orig_coeffs(case.orig)
            else:
                assert_bits_equal(co, case.orig, f"encode_rgb of {case.name}")
            ctx.set_coeffs(case.cand)
            _check_search(ctx, case, w, h, False)
        n += 1
    assert n > 0, only


def case_search_domain_420(L, w, h, only=None):
    """The same on the 4:2:0 frame (search_cases_420), component masks 1 and 6: the original's coefficients come
    from gz_downsample (and must be the oracle's) or go in through gz_set_orig_coeffs_420, case by case in turn."""
    import fields
    n = 0
    for case in fields.search_cases_420(w, h, only):
        with L.context(case.rgb, case.target) as ctx:
            ctx.encode_rgb(download=False)
            if case.foreign or n & 1:
                ctx.set_orig_coeffs_420(case.orig)
            else:
                assert_bits_equal(ctx.downsample(), case.orig, f"downsample of {case.name}")
            ctx.set_coeffs(case.cand)
            _check_search(ctx, case, w, h, True)
        n += 1
    assert n > 0, only


# The candidates the seam is run on: one case per distinct candidate array of the zero_error, saturating (x4 and
# uniform) and foreign_orig families (the seam reads neither the target's cut nor the original coefficients).
SEAM_CASES = ("zero_error/white", "zero_error/black", "zero_error/grey", "saturating/x4",
              "saturating/uniform2040/500.0", "foreign_orig/noise")


def case_compare_blocks_on_search_domain(L, w, h):
    """The per-block seam, coefficient form and pixel form, on candidates of the search cases: 24 random blocks and
    the bottom row and right column of each; on flat white with tiny AC values some errors are exactly 0.0."""
    import fields
    ran = []
    for case in fields.search_cases(w, h, ("zero_error", "saturating", "foreign_orig")):
        if case.name in SEAM_CASES:
            case_compare_blocks(L, w, h, case=case, expect_zero=case.name == "zero_error/white")
            ran.append(case.name)
    assert sorted(ran) == sorted(SEAM_CASES), ran


# ------------------------------------------------ value-domain fields (tests/fields.py) --
BAND_NAMES = ["lf0", "lf1", "lf2", "mf0", "mf1", "mf2", "hf0", "hf1", "uhf0", "uhf1"]
XYB_SCALES = (40.0, -40.0)   # both arms of maximum_clamp on HF-Y, the top of the mask tables


ALL_INSTANTIATIONS = tuple(dict(blur_packed=pk, tile_rows=tr) for pk in (0, 1) for tr in (16, 32))


def _configs(ctx, configs):
    """Walks the context through the given gz_config settings (None: as it is)."""
    base = ctx.get_config().as_dict()
    for cfg in configs:
        if cfg is not None:
            ctx.set_config(**dict(base, **cfg))
        yield "" if cfg is None else f" under {cfg}"
    ctx.set_config(**base)


def case_value_domain_stages(L, w, h, only=None, scaled_xyb=True, configs=(None,)):
    """opsin -> separate_frequencies -> mask -> diffmap against the oracle on every (original,
    candidate) pair of the synthetic fields: the value branches and the device-only arithmetic at
    values a photograph against its mildly quantised copy never produces.  gz_probe_diffmap gets a
    context whose original is the pair's (its mask branch reads the context's precomputed half).
    configs: gz_config settings (blur tile height, packed passes) each pair is probed under; the
    oracle's side is computed once per pair."""
    import fields
    rgb_of_ctx = None
    ctx = None
    try:
        for name, rgb, lin0, lin1 in fields.pairs(w, h, only):
            if ctx is None:
                ctx = L.context(rgb, 1.0)
            elif rgb is not rgb_of_ctx:
                ctx.set_rgb(rgb)
            rgb_of_ctx = rgb
            x0_, x1_ = oracle.opsin(lin0), oracle.opsin(lin1)
            band_in = [(x0_ if name.endswith("/self") else x1_, name)]
            mask_in = [(x0_, x1_, name)]
            if scaled_xyb and name.endswith(("/self", "/inverse")):
                for s in XYB_SCALES:
                    a, b = x0_ * np.float32(s), x1_ * np.float32(s)
                    band_in.append((b, f"{name} x {s}"))
                    mask_in.append((a, b, f"{name} x {s}"))
            band_exp = [oracle.separate_frequencies(x) for x, _ in band_in]
            mask_exp = [oracle.mask(a, b) for a, b, _ in mask_in]
            ed, es = oracle.diffmap(lin0, lin1)
            for under in _configs(ctx, configs):
                assert_bits_equal(ctx.probe_opsin(lin0), x0_, f"opsin(original) of {name}{under}")
                assert_bits_equal(ctx.probe_opsin(lin1), x1_, f"opsin(candidate) of {name}{under}")
                for (x, what), exp in zip(band_in, band_exp):
                    got = ctx.probe_separate_frequencies(x)
                    for i, nm in enumerate(BAND_NAMES):
                        if nm != "mf2":   # dead plane in the reference (wmul[5] == 0), never computed
                            assert_bits_equal(got[i], exp[i], f"separate_frequencies {nm} of {what}{under}")
                for (a, b, what), (em, edc) in zip(mask_in, mask_exp):
                    gm, gdc = ctx.probe_mask(a, b)
                    assert_bits_equal(gm, em, f"mask of {what}{under}")
                    assert_bits_equal(gdc, edc, f"mask_dc of {what}{under}")
                gd, gs = ctx.probe_diffmap(lin0, lin1)
                assert_bits_equal(gd, ed, f"diffmap of {name}{under}")
                assert gs == np.float32(es), name
    finally:
        if ctx is not None:
            ctx.close()


VALUE_DOMAIN_QSCALES = (1, 3, 12, 40)


def case_value_domain_compare(L, w, h, only=None, qscales=VALUE_DOMAIN_QSCALES, target=0.971769, blocks_on=(),
                              configs=(None,)):
    """The production path on every synthetic original: encode_rgb -> quantize(q) -> compare; the
    distance map, the distance, the block maxima and the block weights against the oracle's
    comparator, under each of the gz_config settings.  On the originals named in `blocks_on` also
    phase A's candidate orders and the per-block seam (gz_block_zeroing_orders, gz_compare_blocks)."""
    import fields
    rng = np.random.default_rng(RNG_SEED + 23 * w + h)
    for oname, rgb in fields.originals(w, h).items():
        if only is not None and oname not in only:
            continue
        oc = oracle.comparator(rgb, target)
        with L.context(rgb, target) as ctx:
            co = ctx.encode_rgb()
            assert_bits_equal(co, oracle.encode_rgb(rgb), f"encode_rgb of {oname}")
            for qs in qscales:
                cq = ctx.quantize(np.full((3, 64), qs, np.int32))
                edist, edm = oc.compare(cq)
                pad = np.zeros((ctx.bh * 8, ctx.bw * 8), np.float32)
                pad[:h, :w] = edm
                ebm = pad.reshape(ctx.bh, 8, ctx.bw, 8).max(axis=(1, 3)).reshape(-1)
                ewgt = {d: oc.block_weights(d, 2, 1.0, edm) for d in (1, -1)}
                for under in _configs(ctx, configs):
                    dist, dm, bm = ctx.compare()
                    assert_bits_equal(dm, edm, f"distmap of {oname} q={qs}{under}")
                    assert dist == edist, (oname, qs, under)
                    assert_bits_equal(bm, ebm, f"block max of {oname} q={qs}{under}")
                    for direction in (1, -1):
                        assert_bits_equal(ctx.block_weights(direction, 2, 1.0), ewgt[direction],
                                          f"block weights of {oname} q={qs}{under}")
            if oname in blocks_on:
                cq = ctx.quantize(np.full((3, 64), 3, np.int32))
                off, idx, err = ctx.block_zeroing_orders()
                eoff, eidx, eerr = oc.block_zeroing_orders(cq, co)
                assert_bits_equal(off, eoff, f"candidate offsets of {oname}")
                assert_bits_equal(idx, eidx, f"candidate coefficient indices of {oname}")
                assert_bits_equal(err, eerr, f"candidate errors of {oname}")
                xy, blocks, exp = [], [], []
                for _ in range(12):
                    b = int(rng.integers(0, ctx.nb))
                    cand = cq.copy()
                    for _ in range(int(rng.integers(0, 4))):
                        cand[int(rng.integers(0, 3)), b, int(rng.integers(1, 64))] = 0
                    xy.append((b % ctx.bw, b // ctx.bw))
                    blocks.append(cand[:, b, :])
                    exp.append(oc.compare_block(cand, b % ctx.bw, b // ctx.bw))
                got = ctx.compare_blocks(np.array(xy), np.stack(blocks))
                assert_bits_equal(got, np.array(exp, np.float64), f"CompareBlock of {oname}")
        oc.close()


def case_probe_diffmap_needs_the_contexts_original(L, w=72, h=48):
    """gz_probe_diffmap's documented precondition: rgb0 is the linear image of the context's current
    original (the mask branch reads the half gz_set_rgb precomputed from it).  After gz_set_rgb(other),
    a probe with the matching rgb0 equals the oracle."""
    import fields
    first = images.crop(w, h, 40, 60)
    other = fields.photo_with_zero_rectangle(w, h)
    lin0 = fields.linear(other)
    lin1 = fields.candidates(other)["jpeg_error_x3"]
    ed, es = oracle.diffmap(lin0, lin1)
    with L.context(first, 1.0) as ctx:
        ctx.set_rgb(other)
        gd, gs = ctx.probe_diffmap(lin0, lin1)
        assert_bits_equal(gd, ed, "diffmap after set_rgb(other)")
        assert gs == np.float32(es)
        # and back: the context follows its current original, not the one it was created with
        ctx.set_rgb(first)
        lf = fields.linear(first)
        lc = fields.coded(first)
        gd, gs = ctx.probe_diffmap(lf, lc)
        ed, es = oracle.diffmap(lf, lc)
        assert_bits_equal(gd, ed, "diffmap after set_rgb(first)")
        assert gs == np.float32(es)


def case_stream_choice_same_bits(L, w, h):
    """gz_config.single_stream flipped once on one synthetic field: the same bits."""
    import fields
    rgb = fields.photo_with_zero_rectangle(w, h)
    with L.context(rgb, 0.971769) as ctx:
        ctx.encode_rgb(download=False)
        ctx.quantize(np.full((3, 64), 12, np.int32), download=False)
        base = ctx.get_config().as_dict()
        ctx.set_config(**dict(base, single_stream=1))
        d0, dm0, bm0 = ctx.compare()
        ctx.set_config(**dict(base, single_stream=0))
        d1, dm1, bm1 = ctx.compare()
        assert d0 == d1
        assert_bits_equal(dm1, dm0, "distance map, three streams against one")
        assert_bits_equal(bm1, bm0, "block maxima, three streams against one")


def case_device_math(lib_path, tmp_path, stride, timeout):
    """tests/cpp/test_device_math.cc: the per-pixel functions evaluated by the library at lib_path
    (gz_probe_math) against the plain statement sequences on the host, and div2_shared against the
    device's IEEE division on every stride-th denominator (gz_probe_div2_sweep).  One run under a
    time limit; a non-zero exit fails."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_device_math")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DGZ_EMU",
                    "-I" + os.path.join(root, "guetzli_amd", "csrc"), "-I" + os.path.join(root, "tests", "emu"),
                    os.path.join(root, "tests", "cpp", "test_device_math.cc"), "-o", exe, "-ldl"], check=True)
    out = subprocess.run([exe, lib_path, str(stride)], capture_output=True, text=True, timeout=timeout)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "device_math: ok" in out.stdout
    assert f"div2_shared sweep (stride {stride}):" in out.stdout and " 0 mismatches with the device's division" in out.stdout
    return out.stdout


def case_probe_math_binding(L):
    """Library.probe_math / Library.div2_sweep (capi.py) on a few hundred elements: absent operands,
    the parameter block, two outputs, the int32 form, and the sweep's count and sample layout.  The
    expected values are numpy's IEEE float32 division and C's truncating integer division."""
    rng = np.random.default_rng(RNG_SEED + 77)
    n = 320
    # the production numerators of the first Malta normalisation (butteraugli.cc: 5.1409625726 times and over 0.8)
    n0 = np.full(n, np.float32(5.1409625726 * np.float32(0.8)), np.float32)
    n1 = np.full(n, np.float32(5.1409625726 / np.float32(0.8)), np.float32)
    d = np.exp2(rng.uniform(-40, 40, n)).astype(np.float32)
    got = L.probe_math(0, n0, n1, d, outs=2)                         # GZ_MATH_DIV2_SHARED
    assert got.shape == (2, n)
    assert_bits_equal(got[0], n0 / d, "div2_shared, first quotient")
    assert_bits_equal(got[1], n1 / d, "div2_shared, second quotient")
    # GZ_MATH_MAXIMUM_CLAMP: one operand, one parameter; below the bound the value passes through
    v = rng.uniform(-70.0, 70.0, n).astype(np.float32)
    assert_bits_equal(L.probe_math(5, v, p=(78.8223237675,))[0], v, "maximum_clamp inside its bounds")
    above = L.probe_math(5, np.full(n, 100.0, np.float32), p=(78.8223237675,))[0]
    assert ((above > 78.8223237675) & (above < 100.0)).all()
    # GZ_MATH_QUANT_DIV: int32 operands
    a = rng.integers(-32768, 32768, n).astype(np.int32)
    q = rng.integers(1, 256, n).astype(np.int32)
    want = (np.sign(a) * (np.abs(a) // q)).astype(np.int32)          # C's a / q
    assert_bits_equal(L.probe_math(16, a, q)[0], want, "quant_div")
    # the sweep on every 2^20 + 1-th denominator of [2^-40, 2^40), every sample kept
    num = np.array([n0[0], n1[0]], np.float32)
    stride = (1 << 20) + 1
    bad, sample = L.div2_sweep(num, stride=stride, sample_every=1)
    assert bad == 0
    idx = np.arange(sample.shape[0], dtype=np.uint64) * np.uint64(stride)
    den = ((((idx >> np.uint64(23)) + np.uint64(127 - 40)) << np.uint64(23)) | (idx & np.uint64(0x7fffff)))
    den = den.astype(np.uint32).view(np.float32)
    assert sample.shape == (-(-(80 << 23) // stride), 2)
    assert_bits_equal(sample, num[None, :] / den[:, None], "div2_shared sweep samples")


# ------------------------------------------- the scan coder on tests/entropy_domain.py --
class ContextCache:
    """One context per image size, kept for the cases that follow (their frames and scans reuse its buffers and its
    prefix-scan scratch, as an encode's candidates do); close() at the end of the module."""

    def __init__(self, L):
        self.L, self.ctx = L, {}

    def get(self, w, h):
        if (w, h) not in self.ctx:
            self.ctx[(w, h)] = self.L.context(np.zeros((h, w, 3), np.uint8), 1.0)
        return self.ctx[(w, h)]

    def close(self):
        for c in self.ctx.values():
            c.close()
        self.ctx = {}


def entropy_tables(host, case, kind, counts):
    """(head or None, depth, code) of `kind`; the optimal ones from `counts`, the statistics of the library under test,
    as the product builds them."""
    import entropy_domain as ed
    g = case.geom
    if kind == "optimal":
        return host.jpeg_head(counts, g.w, g.h, case.q, g.ncomp, g.factor)
    depth, code = ed.tables(kind, case.symbols.hist)
    return None, depth, code


def check_entropy_case(ctx, host, case, kind):
    """gz_jpeg_histograms (both kernels) and gz_jpeg_scan (one call, and begin / end) on one case of
    tests/entropy_domain.py under one kind of code table against the reference coder; returns its result."""
    import os
    import entropy_domain as ed
    g, s = case.geom, case.symbols
    what = f"{case.name} {kind} {g.layout} {g.w}x{g.h}"
    ctx.set_frame(g.factor)
    ctx.set_coeffs(case.coeffs)
    assert "GZ_HIST_GENERIC" not in os.environ
    counts = ctx.jpeg_histograms(case.q, g.ncomp)
    assert_bits_equal(counts, s.hist, f"statistics, templated kernel: {what}")
    os.environ["GZ_HIST_GENERIC"] = "1"
    try:
        generic = ctx.jpeg_histograms(case.q, g.ncomp)
    finally:
        del os.environ["GZ_HIST_GENERIC"]
    assert_bits_equal(generic, s.hist, f"statistics, run-time-geometry kernel: {what}")
    head, depth, code = entropy_tables(host, case, kind, counts)
    exp = ed.encode(s, depth, code)
    cap = len(exp.stuffed) + 64
    n = ctx.jpeg_scan(g.ncomp, depth, code)
    scan = ctx.jpeg_scan_bytes(cap=cap)
    assert ctx.jpeg_scan_bits() == (exp.total_bits, exp.stuffed_count), what
    assert n == (exp.total_bits + 7) // 8 + exp.stuffed_count == len(scan), what
    if scan != exp.stuffed:
        got = np.frombuffer(scan, np.uint8)
        want = np.frombuffer(exp.stuffed, np.uint8)
        m = min(got.size, want.size)
        at = int(np.argmax(got[:m] != want[:m])) if (got[:m] != want[:m]).any() else m
        raise AssertionError(f"scan bytes differ from byte {at} of {want.size}: {what}")
    ctx.jpeg_scan_begin(g.ncomp, depth, code)
    assert ctx.jpeg_scan_end() == n, what
    assert ctx.jpeg_scan_bytes(cap=cap) == scan, f"begin / end: {what}"
    assert ctx.jpeg_scan_bits() == (exp.total_bits, exp.stuffed_count), what
    if head is not None:
        assert head + scan + b"\xff\xd9" == host.write_jpeg(case.coeffs, g.w, g.h, case.q, factor=g.factor), what
    return exp


def case_entropy_domain(contexts, host, family, kind, shapes):
    import entropy_domain as ed
    for layout, w, h in shapes:
        check_entropy_case(contexts.get(w, h), host, ed.case(family, layout, w, h), kind)


ENTROPY_KEEP_ORDER = (("dense", "444", "flat16"), ("phase/tiny", "420", "optimal"), ("quant/one", "444", "skewed"),
                      ("sparse", "gray", "optimal"), ("dense", "420", "flat16"))


def case_entropy_keep_across_scans(L, host, w=448, h=296):
    """On ONE context: the longest scan (kept with gz_jpeg_scan_keep), right behind it a much shorter one (a quarter
    of the MCUs: one tile of the prefix scan where there were two, a few hundred bytes where there were hundreds of
    thousands), then long ones again, the unstaged 4:2:0 one among them.  Every scan is checked, and the kept bytes
    are intact after each."""
    import entropy_domain as ed
    with L.context(np.zeros((h, w, 3), np.uint8), 1.0) as ctx:
        kept = None
        sizes = []
        for family, layout, kind in ENTROPY_KEEP_ORDER:
            exp = check_entropy_case(ctx, host, ed.case(family, layout, w, h), kind)
            sizes.append(len(exp.stuffed))
            if kept is None:
                ctx.jpeg_scan_keep()
                kept = exp.stuffed
            assert ctx.jpeg_scan_bytes(kept=True, cap=len(kept) + 64) == kept, f"kept scan after {family} {layout} {kind}"
        assert sizes[0] == max(sizes) and sizes[1] * 100 < sizes[0] and sizes[2] * 4 > sizes[0], sizes


SCAN_PROBE_LENGTHS = (1, 7, 2047, 2048, 2049, 8 * 2048 + 3, 64 * 2048, 64 * 2048 + 1, 65 * 2048 + 1, 130 * 2048 + 77)


def scan_probe_values(name, n):
    rng = np.random.default_rng(RNG_SEED + 77)
    if name == "random":
        return rng.integers(0, 20001, n).astype(np.uint32)
    if name == "zero":
        return np.zeros(n, np.uint32)
    assert name == "2^20-1"     # the total passes 2^32 (from 4097 values on), a tile's sum (2048 of them) stays below 2^31
    return np.full(n, (1 << 20) - 1, np.uint32)


def check_scan_probe(L, values, lengths, start_epoch=0):
    got = L.probe_scan_offsets(values, lengths, start_epoch)
    exp = np.concatenate([[0], np.cumsum(values.astype(np.uint64), dtype=np.uint64)])
    assert len(got) == len(lengths)
    for i, (g, n) in enumerate(zip(got, lengths)):
        assert g.size == n + 1
        if not np.array_equal(g, exp[:n + 1]):
            at = int(np.argmax(g != exp[:n + 1]))
            raise AssertionError(f"launch {i} (n = {n}, epoch after {start_epoch:#x}): off[{at}] = {int(g[at])}, "
                                 f"expected {int(exp[at])}")


def case_scan_probe(L, repeats=20, lengths=SCAN_PROBE_LENGTHS):
    """k_scan_offsets alone (gz_probe_scan_offsets) against numpy.cumsum in uint64: every length of the list in
    ascending order, then long -> short -> long on the same scratch (stale flags of tiles the shorter scan does not
    have), then across the wrap of the flags' epoch field, then the long lengths `repeats` times.

    Which predecessors already hold an inclusive prefix when a tile looks back depends on timing on the GPU, and the
    emulation (workgroups one after the other, in ticket order) always finds it in the nearest one: the test cannot
    choose the arm, it can only give the others the opportunity -- more than 64 and more than 128 tiles, many launches."""
    lengths = list(lengths)
    nmax = max(lengths)
    for name in ("random", "zero", "2^20-1"):
        v = scan_probe_values(name, nmax)
        check_scan_probe(L, v, lengths)
        check_scan_probe(L, v, [lengths[-1], lengths[0], lengths[-1], lengths[4], lengths[-2], lengths[1], lengths[-1]])
        # 0x3ffffffe, then the wrap: cleared, 1, 2, 3 -- long and short across it
        check_scan_probe(L, v, [lengths[-1], lengths[-2], lengths[-1], lengths[2], lengths[-1]], start_epoch=0x3ffffffd)
    v = scan_probe_values("random", nmax)
    long_ones = [n for n in lengths if n > 64 * 2048]
    check_scan_probe(L, v, long_ones * repeats)
    v = scan_probe_values("2^20-1", nmax)
    check_scan_probe(L, v, long_ones * repeats)


# ------------------------------------------------ phase B on tests/order_domain.py --
class TargetContexts:
    """One context per (size, target, tag), kept for the cases that follow; close() at the end of the module."""

    def __init__(self, L):
        self.L, self.ctx = L, {}

    def get(self, w, h, target, tag=""):
        key = (w, h, float(target), tag)
        if key not in self.ctx:
            self.ctx[key] = self.L.context(np.zeros((h, w, 3), np.uint8), target)
        return self.ctx[key]

    def close(self):
        for c in self.ctx.values():
            c.close()
        self.ctx = {}


def _order_frame(ctx, g):
    factor = 2 if g.layout == "420" else 1
    if ctx.cfac != factor or getattr(ctx, "_od_frame", None) != factor:
        ctx.set_frame(factor)
        ctx._od_frame, ctx._od_search = factor, None


def _install_search(ctx, g, key, off, idx, err):
    """gz_probe_set_search, once for the cases that share `key` on this context."""
    _order_frame(ctx, g)
    if key is None or getattr(ctx, "_od_search", None) != (g.mask, key):
        ctx.probe_set_search(off, idx, err, comp_mask=g.mask)
        ctx._od_search = (g.mask, key)


def _unit_search(ctx, g):
    """One candidate of error 1 per block: an order holds the blocks of non-zero weight, their weights in its vals."""
    off = np.arange(g.gn + 1, dtype=np.int32)
    _install_search(ctx, g, "unit", off, np.ones(g.gn, np.uint8), np.ones(g.gn, np.float32))
    return off, np.ones(g.gn, np.float32)


def _check_order(ctx, got_counts, exp, what, permuted=False):
    """(total, blocks_to_change, below) and the entries of the context's order against build_order's."""
    eb, ev, btc, below = exp
    assert got_counts == (eb.size, btc, below), (what, got_counts, (eb.size, btc, below))
    got = ctx.order_fetch(0, eb.size)
    if permuted:       # behind a descent: the same entries, rearranged
        key = lambda b, v: np.lexsort((b, v.view(np.uint32)))
        i, j = key(got["block"], got["val"]), key(eb, ev)
        assert_bits_equal(got["block"][i], eb[j], what + ": blocks (as a set)")
        assert_bits_equal(got["val"][i], ev[j], what + ": vals (as a set)")
    else:
        assert_bits_equal(got["block"], eb, what + ": blocks")
        assert_bits_equal(got["val"], ev, what + ": vals")
    return got


def check_weight_case(ctx, case, host_form=False):
    """k_block_max_group / k_weights_flag / k_weights_gather through gz_order_build_auto at every radius, direction
    and target_mul: the device's weights bit for bit, and the order they select."""
    import order_domain as od
    g = case.g
    off, err = _unit_search(ctx, g)
    ctx.probe_set_block_max(case.bmax8)
    for direction in (1, -1):
        nc = np.zeros(g.gn, np.int32) if direction > 0 else np.ones(g.gn, np.int32)
        for r in od.RADII:
            for mul in od.MULS:
                what = f"{case.family} {g.name} target {case.target} direction {direction} r {r} mul {mul}"
                exp = case.reference(direction, r, mul)
                counts = ctx.order_build_auto(direction, r, mul, case.use_distmap, nc, limit=0.5)
                wgt, me = ctx.probe_order_state()
                assert_bits_equal(wgt, exp, "weights: " + what)
                _check_order(ctx, counts, od.build_order(off, err, nc, me, exp, direction, 0.5), what)
                if host_form:
                    f = ctx.block_weights_factor(direction, r, mul, g.factor, case.use_distmap)
                    assert_bits_equal(f, exp, "gz_block_weights_factor: " + what)


def case_order_weights(contexts, family, grid_index, target, host_form=False):
    import order_domain as od
    g = od.WEIGHT_GRIDS[grid_index]
    ctx = contexts.get(g.w, g.h, target)
    ctx.order_reset()
    for case in od.weight_cases(family, g, target):
        check_weight_case(ctx, case, host_form)


def check_order_case(ctx, case):
    """One input through gz_order_build (host weights), gz_order_build_auto, _begin / _end and the fused
    _descend_begin: the same entries from all four."""
    import order_domain as od
    g = case.g
    what = f"{case.family} {g.name} direction {case.direction}"
    _install_search(ctx, g, None, case.off, case.idx, case.err)
    ctx.probe_set_block_max(case.bmax8)
    wgt = case.weights()
    exp = case.reference()
    lim = case.limit
    args = (case.direction, case.r, case.mul, True, case.next_cand)
    _check_order(ctx, ctx.order_build(case.direction, case.next_cand, case.max_err, wgt, limit=lim), exp,
                 what + ": gz_order_build")
    _check_order(ctx, ctx.order_build_auto(*args, limit=lim), exp, what + ": gz_order_build_auto")
    dw, dme = ctx.probe_order_state()
    assert_bits_equal(dw, wgt, what + ": device weights")
    assert_bits_equal(dme, case.max_err, what + ": max_block_error")
    ctx.order_build_auto_begin(*args, limit=lim)
    _check_order(ctx, ctx.order_build_auto_end(), exp, what + ": _begin / _end")
    per_block = 2.0 if case.direction > 0 else 0.2
    ctx.order_build_auto_descend_begin(*args, per_block, 16, 12, limit=lim)
    counts = ctx.order_build_auto_end()
    log, last = ctx.order_descend_end()
    got = _check_order(ctx, counts, exp, what + ": _descend_begin", permuted=True)
    n = exp[0].size
    if n > 16:
        assert len(log) > 0 and last == od.derived_last(per_block, exp[2], n), (what, last, exp[2], n)
        for lo, hi, cut in log.astype(np.int64):     # each cut parts its range
            assert lo < cut <= hi and (cut == hi or got["val"][lo:cut].max() <= got["val"][cut:hi].min()), (what, lo, hi, cut)
    else:
        assert len(log) == 0 and last == 0, what


def case_order_build(contexts, family):
    import order_domain as od
    for case in od.order_cases(family):
        check_order_case(contexts.get(case.g.w, case.g.h, case.target), case)


def case_order_advance(contexts, family):
    """gz_order_advance: the update rides on the next gz_order_build_auto's k_weights_gather with the weights that
    kernel replaces, once; two in a row; dropped by gz_order_build."""
    import order_domain as od
    g = od.grid_of_blocks(17, 13)
    target = od.TARGETS[0]
    ctx = contexts.get(g.w, g.h, target)
    off, err = _unit_search(ctx, g)
    A = np.full((g.bh, g.bw), 0.25 * target, np.float32)
    A[3, 4] = A[9, 12] = 3 * target
    B = np.full((g.bh, g.bw), 0.25 * target, np.float32)
    B[6, 8] = 3 * target
    ones = np.ones(g.gn, np.int32)
    wA = od.weights_of(g, A, target, -1, 2, 1.0)
    wB1, wB2 = (od.weights_of(g, B, target, -1, r, 1.0) for r in (1, 2))
    assert (wA != wB2).any() and (wB1 != wB2).any()
    thr, thr2 = np.float32(0.3125 + 1e-3), np.float32(0.07)

    def start():
        ctx.order_reset()
        ctx.probe_set_block_max(A)
        ctx.order_build_auto(-1, 2, 1.0, True, ones)
        w, me = ctx.probe_order_state()
        assert_bits_equal(w, wA, "weights before the advance")
        assert not me.any()
        return me

    def state_is(w, me, what):
        gw, gme = ctx.probe_order_state()
        assert_bits_equal(gw, w, family + ": weights " + what)
        assert_bits_equal(gme, me, family + ": max_block_error " + what)
    me = start()
    if family == "advance/fused":
        ctx.order_advance(float(thr), -1)
        ctx.probe_set_block_max(B)
        counts = ctx.order_build_auto(-1, 2, 1.0, True, ones)
        me = od.advance(me, wA, thr, -1)
        _check_order(ctx, counts, od.build_order(off, err, ones, me, wB2, -1), family)     # (read AFTER the build)
        state_is(wB2, me, "after the build that carries the advance")
    elif family == "advance/escalate":
        gy, gx = np.mgrid[0:g.bh, 0:g.bw]
        ring2 = (np.maximum(abs(gy - 6), abs(gx - 8)) == 2).reshape(-1)
        nc = ring2.astype(np.int32)                     # applied candidates only at distance 2 of the hot block
        ctx.order_advance(float(thr), -1)
        ctx.probe_set_block_max(B)
        assert ctx.order_build_auto(-1, 1, 1.0, True, nc)[0] == 0          # radius 1: an empty order
        counts = ctx.order_build_auto(-1, 2, 1.0, True, nc)                # radius 2
        me = od.advance(me, wA, thr, -1)                                   # once, with the OLD weights
        exp = od.build_order(off, err, nc, me, wB2, -1)
        assert exp[0].size == ring2.sum() > 0
        _check_order(ctx, counts, exp, family)
        state_is(wB2, me, "after the escalation")
    elif family == "advance/twice":
        ctx.order_advance(float(thr), -1)
        ctx.order_advance(float(thr2), 1)
        ctx.probe_set_block_max(B)
        counts = ctx.order_build_auto(-1, 2, 1.0, True, ones)
        me = od.advance(od.advance(me, wA, thr, -1), wA, thr2, 1)
        _check_order(ctx, counts, od.build_order(off, err, ones, me, wB2, -1), family)
        state_is(wB2, me, "after two advances")
        ctx.order_advance(float(thr2), -1)                                 # ... and read without a build: made first
        state_is(wB2, od.advance(me, wB2, thr2, -1), "flushed by the read")
    elif family == "advance/replaced":
        ctx.order_advance(float(thr), -1)
        rng = np.random.default_rng(5)
        hw = rng.choice(np.array([0, 1, 0.5, 1 / 3], np.float32), g.gn)
        hme = rng.random(g.gn).astype(np.float32)
        counts = ctx.order_build(-1, ones, hme, hw)
        _check_order(ctx, (counts[0], counts[1], 0), od.build_order(off, err, ones, hme, hw, -1), family)
        state_is(hw, hme, "after gz_order_build replaced the state")
    else:
        raise KeyError(family)


def check_step_case(ctx, case):
    """gz_apply_candidate_steps + gz_steps_histogram_delta (k_apply_steps_hist / k_steps_hist_sum), or k_apply_steps on
    a context that has no statistics quantiser: coefficients and the AC statistics change, call by call."""
    g = case.g
    _order_frame(ctx, g)
    ctx._od_search = None
    (ctx.set_orig_coeffs_420 if g.layout == "420" else ctx.set_orig_coeffs)(case.layout(case.orig))
    ctx._od_frame = ctx.cfac
    ctx.quantize(case.q, download=False)                 # the steps' quantiser
    ctx.set_coeffs(case.layout(case.cand))
    ctx.probe_set_search(case.off, case.idx, np.zeros(case.idx.size, np.float32), comp_mask=g.mask)
    if case.with_statistics:
        ctx.jpeg_histograms(case.q)                      # the symbols' quantiser
    zero_w, zero_e = np.zeros(g.gn, np.float32), np.zeros(g.gn, np.float32)
    for i, ((direction, next_cand, blocks, counts, read), (exp, exp_delta)) in enumerate(zip(case.calls, case.reference())):
        what = f"{case.family} {g.name} call {i} direction {direction} n {len(blocks)}"
        ctx.order_build(direction, next_cand, zero_e, zero_w)        # uploads next_cand (an empty order)
        ctx.apply_candidate_steps(direction, blocks, counts)
        if read and case.with_statistics:
            assert_bits_equal(ctx.steps_histogram_delta(), exp_delta, "statistics change: " + what)
        assert_bits_equal(ctx.get_coeffs().reshape(-1, 64), exp, "coefficients: " + what)


def case_order_steps(L, contexts, family):
    import order_domain as od
    for case in od.step_cases(family):
        g = case.g
        if case.with_statistics:
            check_step_case(contexts.get(g.w, g.h, 1.0, "steps"), case)
        else:       # k_apply_steps: a context no gz_jpeg_histograms has given a statistics quantiser
            with L.context(np.zeros((g.h, g.w, 3), np.uint8), 1.0) as ctx:
                check_step_case(ctx, case)


def case_order_descent(contexts, per_block, big, short=False, log_every=1, every=1):
    """The position gz_order_descend_begin derives on the device == the reference's, and its cut log == that of
    gz_order_descend with that position on a second context that never derived one."""
    import order_domain as od
    g = od.Grid(*od.BIG) if big else od.grid_of_blocks(17, 13)
    a, b = contexts.get(g.w, g.h, 1.0, "descent"), contexts.get(g.w, g.h, 1.0, "descent/plain")
    search = od.descent_search(g)
    for c in (a, b):
        _install_search(c, g, "descent", *search)
    values = od.btc_values(per_block, g.gn)
    if big:
        values = [v for v in values if v > 221]
    if short:
        values = [v for v in values if v <= 60 or v % 7 == 0]
    values = values[::every]       # (the emulation: a sample of the large context's values)
    for i, btc in enumerate(values):
        nc = od.descent_next_cand(g, btc, short)
        n = btc * (1 if short else od.DESCENT_CNT)
        a.order_build_auto_begin(1, 1, 1.0, False, nc)
        a.order_descend_begin(per_block, 16, 12)
        total, got_btc, _ = a.order_build_auto_end()
        log, last = a.order_descend_end()
        assert (total, got_btc) == (n, btc), (per_block, btc, total, got_btc)
        if n <= 16:
            assert len(log) == 0 and last == 0, (per_block, btc)
            continue
        assert len(log) > 0 and last == od.derived_last(per_block, btc, n), (per_block, btc, n, last)
        if i % log_every == 0:
            b.order_build_auto(1, 1, 1.0, False, nc)
            log2 = b.order_descend(last, 16, 12)
            assert_bits_equal(log, log2, f"cut log, per_block {per_block} blocks_to_change {btc}")
            assert_bits_equal(a.order_fetch(0, n), b.order_fetch(0, n), f"order after the descent, {per_block} {btc}")


# ------------------------------------------------ the frame path on tests/frame_domain.py --
# Pixels -> coefficients -> pixels on synthetic families (tests/test_frame_domain.py counts the arms they take with the
# oracle's frame_* census; tests/test_frame_gpu.py runs these cases on the GPU).  Integers and float bit patterns only.
def frame_context(contexts, w, h):
    """The frame cases' context of this size, with the patches' self-check on (gz_config.patch_reconstruct = 2: a Compare
    that relies on patched planes compares them, word for word, with a full reconstruction first)."""
    ctx = contexts.get(w, h, 1.0, "frame")
    ctx.set_config(patch_reconstruct=2)
    return ctx


def case_frame_encode(L, contexts, sizes):
    """k_encode_rgb with and without a context: the lattice of colours, and the pixel families at sizes that replicate
    one and seven columns / rows."""
    import frame_domain as fd
    img = fd.lattice_image()
    assert_bits_equal(L.encode_rgb_only(img), oracle.encode_rgb(img), "encode_rgb_only lattice")
    for w, h in sizes:
        for name, rgb in fd.pixel_cases(w, h):
            exp = oracle.encode_rgb(rgb)
            assert_bits_equal(L.encode_rgb_only(rgb), exp, f"encode_rgb_only {name} {w}x{h}")
            if w >= 8 and h >= 8:
                ctx = frame_context(contexts, w, h)
                ctx.set_rgb(rgb)
                assert_bits_equal(ctx.encode_rgb(), exp, f"encode_rgb {name} {w}x{h}")


def _frame_block_list(nb):
    """Block positions for a patching call: repeats (adjacent and not), the first and the last block; at most nb / 2
    entries, beyond which the library leaves the planes to the next full reconstruction."""
    return np.array([0, 0, nb - 1, nb // 2, 0, nb - 1, nb - 1, nb // 3][:nb // 2], np.int32)


def _frame_patched_planes(L, ctx, co, w, h, what):
    """k_reconstruct_listed on the family's blocks: bulk steps (gz_apply_candidate_steps, block positions) and
    single-coefficient edits (gz_apply_coeff_edits, coefficient positions) with lists that hold repeats and the first
    and last block; the Compare that follows checks the patched planes against a full reconstruction itself (mode 2)
    and must give what a Compare of the same coefficients put in place as a whole gives."""
    import order_domain as od
    nb = ctx.nb
    g = od.Grid(w, h)
    ones = np.ones((3, 64), np.int32)
    rng = np.random.default_rng(RNG_SEED + 13 * w + h)
    ctx.set_orig_coeffs(co)
    ctx.quantize(ones, download=False)             # the candidate = the family's coefficients
    # one candidate per block: coefficient 2..63 but 8 (positions 1 and 8 may be kept as "precious") of a component
    k = rng.integers(2, 64, nb)
    k[k == 8] = 9
    idx = (64 * rng.integers(0, 3, nb) + k).astype(np.uint8)
    off = np.arange(nb + 1, dtype=np.int32)
    ctx.probe_set_search(off, idx, np.zeros(nb, np.float32))
    ctx.jpeg_histograms(ones)
    ctx.compare()                                   # a full reconstruction: the planes are the candidate's
    next_cand = np.zeros(nb, np.int32)
    ctx.order_build(1, next_cand, np.zeros(nb, np.float32), np.zeros(nb, np.float32))   # (uploads next_cand)
    blocks = _frame_block_list(nb)
    before = L.compare_counters()
    exp = np.asarray(co, np.int16).reshape(-1, 64).copy()
    if blocks.size:
        ctx.apply_candidate_steps(1, blocks, np.ones(blocks.size, np.int32))
        ctx.steps_histogram_delta()
        exp = od.apply_steps(g, exp, co, ones, off, idx, next_cand, 1, blocks, np.ones(blocks.size, np.int32))
        eb = blocks[::-1].copy()                    # (the same positions, in another order, as coefficient positions)
        pos = ((rng.integers(0, 3, eb.size) * nb + eb) * 64 + rng.integers(0, 64, eb.size)).astype(np.int32)
        val = np.array([32767, -32768, 16384, -16384, 1, 0, -1, 8191], np.int16)[:eb.size]
        ctx.apply_coeff_edits(pos, val)
        for p, v in zip(pos, val):                  # (in order: a later edit of the same position wins)
            exp.reshape(-1)[p] = v
    import frame_domain as fd
    assert fd.idct_sums_fit_int32(exp)
    got = ctx.compare()
    patched, checked, compares = (a - b for a, b in zip(L.compare_counters(), before))
    # (no list at all on a frame of one block: the planes of the Compare before are still the candidate's)
    assert (patched, checked, compares) == (1, 1, 1), (what, patched, checked, compares)
    assert_bits_equal(ctx.get_coeffs().reshape(-1, 64), exp, f"coefficients after steps and edits: {what}")
    ctx.set_coeffs(exp)
    full = ctx.compare()
    for a, b, name in zip(got, full, ("distance", "distance map", "block maxima")):
        assert_bits_equal(np.asarray(a, np.float32), np.asarray(b, np.float32), f"patched {name}: {what}")
    _, esrgb, elin = oracle.reconstruct(exp.reshape(3, nb, 64), w, h, None)
    srgb, lin = ctx.reconstruct()
    assert_bits_equal(srgb, esrgb, f"reconstruct srgb after steps and edits: {what}")
    assert_bits_equal(lin, elin, f"reconstruct linear after steps and edits: {what}")


def case_frame_coeffs444(L, contexts, w, h, family, tables=None, patched=True):
    """gz_set_orig_coeffs -> gz_quantize -> gz_reconstruct (sRGB and linear), gz_decode_coeffs, gz_set_coeff_blocks and
    the patched planes on a coefficient family, under every quantiser table."""
    import frame_domain as fd
    co = fd.coeffs_of(family, w, h, "444")
    assert fd.idct_sums_fit_int32(co), "the family's IDCT sums leave int32"
    ctx = frame_context(contexts, w, h)
    ctx.set_orig_coeffs(co)
    ecq = None
    for qn, q in fd.quant_tables(co, "444", w, h, only=tables):
        what = f"{family} q={qn} 444 {w}x{h}"
        cq = ctx.quantize(q)
        ecq, esrgb, elin = oracle.reconstruct(co, w, h, q)
        assert fd.idct_sums_fit_int32(ecq)
        assert_bits_equal(cq, fd.quantize_by_definition(co, q, "444", w, h), f"quantize, block by block: {what}")
        assert_bits_equal(cq, ecq, f"quantize: {what}")
        srgb, lin = ctx.reconstruct()
        assert_bits_equal(srgb, esrgb, f"reconstruct srgb: {what}")
        assert_bits_equal(lin, elin, f"reconstruct linear: {what}")
        assert_bits_equal(L.decode_coeffs(ecq, w, h, 1), esrgb, f"decode_coeffs: {what}")
    # block updates: the first, the middle and the last block replaced by the wrap family's
    idx = np.unique(np.array([0, ctx.nb - 1, ctx.nb // 2], np.int32))
    other = fd.coeffs_of("wrap", w, h, "444")
    ctx.set_coeff_blocks(idx, np.ascontiguousarray(other[:, idx].transpose(1, 0, 2)))
    exp = ecq.copy()
    exp[:, idx] = other[:, idx]
    assert_bits_equal(ctx.get_coeffs(), exp, f"set_coeff_blocks: {family} {w}x{h}")
    _, esrgb, elin = oracle.reconstruct(exp, w, h, None)
    srgb, lin = ctx.reconstruct()
    assert_bits_equal(srgb, esrgb, f"reconstruct srgb after set_coeff_blocks: {family} {w}x{h}")
    assert_bits_equal(lin, elin, f"reconstruct linear after set_coeff_blocks: {family} {w}x{h}")
    if patched:
        _frame_patched_planes(L, ctx, co, w, h, f"{family} {w}x{h}")


def case_frame_coeffs420(L, contexts, w, h, family, tables=None):
    """gz_set_orig_coeffs_420 -> gz_quantize (component boundaries nb, nb + nbc) -> gz_reconstruct (k_chroma_samples,
    k_reconstruct420), and gz_decode_coeffs with factor 2 equal to reconstruct's bytes."""
    import frame_domain as fd
    co = fd.coeffs_of(family, w, h, "420")
    assert fd.idct_sums_fit_int32(co), "the family's IDCT sums leave int32"
    ctx = frame_context(contexts, w, h)
    ctx.set_orig_coeffs_420(co)
    assert ctx.frame_layout() == (2, ctx.nb, ctx.nbc)
    for qn, q in fd.quant_tables(co, "420", w, h, only=tables):
        what = f"{family} q={qn} 420 {w}x{h}"
        cq = ctx.quantize(q)
        ecq, esrgb, elin = oracle.reconstruct420(co, w, h, q, shuffle=7)
        assert fd.idct_sums_fit_int32(ecq)
        assert_bits_equal(cq, fd.quantize_by_definition(co, q, "420", w, h), f"quantize, block by block: {what}")
        assert_bits_equal(cq, ecq, f"quantize: {what}")
        srgb, lin = ctx.reconstruct()
        assert_bits_equal(srgb, esrgb, f"reconstruct srgb: {what}")
        assert_bits_equal(lin, elin, f"reconstruct linear: {what}")
        assert_bits_equal(L.decode_coeffs(ecq, w, h, 2), srgb, f"decode_coeffs == reconstruct: {what}")


def frame_downsample_inputs(w, h):
    """(name, 4:4:4 coefficients) for gz_downsample: the YUV fields, the photograph, and the two coefficient families whose
    pixels stay near [0, 255] (ToFloatPixels does not clamp: the others' samples are beyond what a rounded coefficient
    of SetDownsampledCoefficients can hold)."""
    import frame_domain as fd
    yield from fd.yuv_cases(w, h)
    for name in ("photo", "dc_ramp", "chroma_extreme"):
        yield name, fd.coeffs_of(name, w, h, "444")


def case_frame_downsample(L, contexts, w, h):
    """gz_component_to_float_pixels and gz_downsample (k_to_float_pixels, the nine k_pp_* kernels,
    k_set_downsampled_coeffs by 2 x 2) on foreign 4:4:4 coefficients."""
    ctx = frame_context(contexts, w, h)
    for name, co in frame_downsample_inputs(w, h):
        what = f"{name} {w}x{h}"
        assert np.asarray(co)[1:].any(), "a grey frame stays 4:4:4"
        for c in range(3):
            assert_bits_equal(L.component_to_float_pixels(co[c], w, h), oracle.to_float_pixels(co[c], w, h),
                              f"ToFloatPixels c={c}: {what}")
        exp = oracle.downsample(co, w, h)
        # (the cast of a rounded double outside int16 is undefined in the reference)
        assert np.abs(exp.astype(np.int32)).max() < 32767, what
        ctx.set_orig_coeffs(co)
        got = ctx.downsample()
        assert ctx.frame_layout() == (2, ctx.nb, ctx.nbc)
        assert_bits_equal(got, exp, f"downsample: {what}")


def case_frame_planes(L):
    """gz_component_set_downsampled for every (fx, fy) in 1..4 squared: source clamps at sizes that are no multiple of
    8 fx / 8 fy (w < fx and a single row among them), samples outside [0, 255], and the rounding ties."""
    import frame_domain as fd
    for w, h in fd.PLANE_SIZES:
        for name, p in fd.plane_cases(w, h):
            lo, hi = fd.PLANE_RANGE
            assert lo <= p.min() and p.max() <= hi
            for fx, fy in fd.FACTORS:
                assert_bits_equal(L.component_set_downsampled(p, fx, fy), oracle.set_downsampled(p, fx, fy),
                                  f"SetDownsampledCoefficients {name} {w}x{h} by {fx}x{fy}")
    for name, p, fx, fy in fd.tie_planes():
        exp = oracle.set_downsampled(p, fx, fy)
        t = float(name.split("/")[1])
        assert exp[0, 0] == (t + 0.5 if t > 0 else t - 0.5), (name, exp[0, 0])   # half away from zero
        assert_bits_equal(L.component_set_downsampled(p, fx, fy), exp, f"SetDownsampledCoefficients {name}")
    for name, p in fd.constant_planes():
        for fx, fy in ((1, 1), (2, 2)):
            assert_bits_equal(L.component_set_downsampled(p, fx, fy), oracle.set_downsampled(p, fx, fy),
                              f"SetDownsampledCoefficients {name} by {fx}x{fy}")


def case_frame_free_sizes(L):
    """The context-free entries below 8 pixels: gz_component_to_float_pixels and gz_decode_coeffs in both chroma
    factors on the extreme families."""
    import frame_domain as fd
    for w, h in fd.FREE_SIZES:
        for family in ("sparse", "matrix_rows", "wrap", "chroma_extreme"):
            co = fd.coeffs_of(family, w, h, "444")
            for c in range(3):
                assert_bits_equal(L.component_to_float_pixels(co[c], w, h), oracle.to_float_pixels(co[c], w, h),
                                  f"ToFloatPixels {family} c={c} {w}x{h}")
            assert_bits_equal(L.decode_coeffs(co, w, h, 1), oracle.reconstruct(co, w, h, None)[1],
                              f"decode_coeffs 444 {family} {w}x{h}")
            co2 = fd.coeffs_of(family, w, h, "420")
            assert_bits_equal(L.decode_coeffs(co2, w, h, 2), oracle.reconstruct420(co2, w, h, None)[1],
                              f"decode_coeffs 420 {family} {w}x{h}")


def case_frame_idct_copies(L, contexts, w, h):
    """The copies of the integer IDCT against each other, no oracle: the same luma blocks (sparse, matrix rows, wrap)
    under flat chroma (all chroma coefficients 0: Cb = Cr = 128, R = G = B = Y) through k_reconstruct (packed 16-bit
    dot products), k_reconstruct420 (24-bit multiplies), k_idct_blocks, and k_reconstruct_listed (every block listed
    once, at most half of them per call: the library's own word-for-word check against k_reconstruct, mode 2)."""
    import frame_domain as fd
    ctx = frame_context(contexts, w, h)
    nb, nbc, bw = ctx.nb, ctx.nbc, ctx.bw
    yb = fd.luma_extreme_blocks(nb, shift=w + h)
    px = L.idct_blocks(yb)
    pad = px.reshape(ctx.bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(ctx.bh * 8, bw * 8)[:h, :w]
    ref_px, bound, wrapped = fd.idct_blocks_int64(yb)
    assert bound < (1 << 31) and (nb < 3 or wrapped > 0)
    assert_bits_equal(px, ref_px, "idct_blocks against the int64 evaluation")
    grey = np.repeat(pad[:, :, None], 3, axis=2)
    co444 = np.zeros((3, nb, 64), np.int16)
    co444[0] = yb
    ctx.set_orig_coeffs(co444)
    ctx.quantize(None, download=False)
    s444, l444 = ctx.reconstruct()
    assert_bits_equal(s444, grey, f"k_reconstruct against k_idct_blocks {w}x{h}")
    # every block through k_reconstruct_listed: an edit that writes the value already there, half the blocks per call
    ctx.compare()
    before = L.compare_counters()
    halves = [np.arange(s, min(s + nb // 2, nb)) for s in range(0, nb, nb // 2)] if nb >= 2 else []
    for half in halves:
        pos = (half * 64 + 63).astype(np.int32)
        ctx.apply_coeff_edits(pos, yb[half, 63])
        ctx.compare()
    patched, checked, _ = (a - b for a, b in zip(L.compare_counters(), before))
    assert patched == checked == len(halves)
    co420 = np.zeros((nb + 2 * nbc, 64), np.int16)
    co420[:nb] = yb
    ctx.set_orig_coeffs_420(co420)
    ctx.quantize(None, download=False)
    s420, l420 = ctx.reconstruct()
    assert_bits_equal(s420, grey, f"k_reconstruct420 against k_idct_blocks {w}x{h}")
    assert_bits_equal(l420, l444, f"k_reconstruct420 against k_reconstruct, linear {w}x{h}")


def recon_strips_per_workgroup(w, h):
    """stage_reconstruct's rule (chain.h): as many strips of 8 blocks per workgroup, up to 4, as leave 2000 workgroups."""
    bw, bh = (w + 7) // 8, (h + 7) // 8
    strips = -(-bw // 8)
    per = 4
    while per > 1 and bh * -(-strips // per) < 2000:
        per >>= 1
    return per


def case_frame_strips(L, w, h):
    """k_reconstruct's strip loop on the mixed synthetic coefficients, sRGB and linear."""
    import frame_domain as fd
    co = fd.mixed_coeffs(w, h)
    assert fd.idct_sums_fit_int32(co)
    _, esrgb, elin = oracle.reconstruct(co, w, h, None)
    with L.context(np.zeros((h, w, 3), np.uint8), 1.0) as ctx:
        ctx.set_orig_coeffs(co)
        ctx.quantize(None, download=False)
        srgb, lin = ctx.reconstruct()
        assert_bits_equal(srgb, esrgb, f"reconstruct srgb {w}x{h}")
        assert_bits_equal(lin, elin, f"reconstruct linear {w}x{h}")
