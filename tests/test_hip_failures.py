"""Out-of-memory and launch-failure paths of the C ABI and of the host driver above it (VERDICT r5 "HIP-failure paths
are untested").

The CPU emulation's hipMalloc / hipHostMalloc (tests/emu/hip_emu.h) count every allocation, can be told to fail the
n-th one from now on with hipErrorOutOfMemory, and list what is still allocated.  Its kernel launches are counted the
same way, and the n-th one from now on can be made to fail.  Checked here:
  * gz_create with EVERY one of its allocations failing in turn: NULL + GZ_E_NOMEM, nothing left allocated (device
    blocks, page-locked blocks, events), and the next gz_create succeeds;
  * a whole encode through the host driver with allocations failing at sampled points of its life (context creation,
    block search, phase B's order, the entropy coder's buffers, staging): the encode fails with an error -- no crash,
    nothing left allocated -- and the encode after it produces the reference's bytes;
  * the calls that write the candidate or the original with EVERY one of their launches failing in turn: the call
    fails, and a caller that goes on gets a Compare that does not trust planes the failed call may have left stale
    (the context's claims, context.h), with the distance of a fresh context given the same coefficients -- or, after a
    failed downsample, a refusal to quantize a half-written original.
  * every entry point that makes buffers on first use, with EVERY one of its allocations failing in turn, and the
    first order, block search and scan with every asynchronous copy or fill failing: the call fails, the SAME context
    repeats it with the clean call's results bit for bit, and gz_destroy leaves nothing allocated.
(The emulation build allocates directly instead of through the product's pools, so "still allocated" is exact.)
CPU only."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

import images
from checkers import assert_bits_equal, ref
from guetzli_amd.capi import GuetzliAmdError, Library

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import build_emu  # noqa: E402

GZ_E_NOMEM = -5


@pytest.fixture(scope="module")
def emu():
    lib = C.CDLL(build_emu.build())
    lib.gz_create.restype = C.c_void_p
    lib.gz_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.POINTER(C.c_int)]
    lib.gz_destroy.argtypes = [C.c_void_p]
    lib.gz_emu_fail_alloc.argtypes = [C.c_long]
    lib.gz_emu_alloc_calls.restype = C.c_long
    lib.gz_emu_live.argtypes = [C.POINTER(C.c_long)] * 4
    lib.gz_emu_fail_launch.argtypes = [C.c_long]
    lib.gz_emu_launch_calls.restype = C.c_long
    return lib


def live(lib):
    v = [C.c_long() for _ in range(4)]
    lib.gz_emu_live(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)   # device bytes, page-locked bytes, blocks, events


def test_gz_create_survives_every_allocation_failing(emu):
    rgb = np.ascontiguousarray(images.crop(40, 32, 100, 60))
    err = C.c_int(0)
    base = live(emu)
    before = emu.gz_emu_alloc_calls()
    ctx = emu.gz_create(0, 40, 32, rgb.ctypes.data, 0.971769, C.byref(err))
    assert ctx and err.value == 0
    n_allocs = emu.gz_emu_alloc_calls() - before
    assert n_allocs >= 15, n_allocs          # the arena, the coefficient arrays, tables, blur scales, staging ...
    emu.gz_destroy(ctx)
    assert live(emu) == base, "a clean create / destroy leaves allocations behind"
    for n in range(n_allocs):
        emu.gz_emu_fail_alloc(n)
        ctx = emu.gz_create(0, 40, 32, rgb.ctypes.data, 0.971769, C.byref(err))
        assert not ctx, f"gz_create succeeded although allocation {n} failed"
        assert err.value == GZ_E_NOMEM, (n, err.value)
        assert live(emu) == base, f"allocation {n} failing leaves {live(emu)} (device bytes, host bytes, blocks, events)"
        emu.gz_emu_fail_alloc(-1)
        ctx = emu.gz_create(0, 40, 32, rgb.ctypes.data, 0.971769, C.byref(err))
        assert ctx and err.value == 0, f"gz_create after the failure of allocation {n}"
        emu.gz_destroy(ctx)
        assert live(emu) == base


@pytest.mark.skipif(ref is None, reason="oracle/_ref/libgz_ref.so not built")
def test_an_encode_survives_allocations_failing_anywhere(emu):
    """The host driver over the same library: allocation k of an encode fails -> Process fails cleanly."""
    from guetzli_amd.encoder import HostLibrary
    host = HostLibrary(build_emu.build_host())
    rgb = np.ascontiguousarray(images.crop(40, 32, 100, 60))
    exp = hashlib.sha256(ref.process(rgb, ref._butteraugli_score_for_quality(90.0))[0]).hexdigest()
    base = live(emu)
    before = emu.gz_emu_alloc_calls()
    jpg, _ = host.process(rgb, quality=90.0)
    assert hashlib.sha256(jpg).hexdigest() == exp
    total = emu.gz_emu_alloc_calls() - before
    assert live(emu) == base, "a clean encode leaves allocations behind"
    assert total >= 40, total
    # every allocation of the first 60 (context, first calls of every entry point), then every seventh
    points = sorted(set(range(min(60, total))) | set(range(60, total, 7)) | {total - 1})
    failed = 0
    for k in points:
        emu.gz_emu_fail_alloc(k)
        try:
            out, _ = host.process(rgb, quality=90.0)
            # an allocation that the encode can do without (a cache, an optional buffer) may be survived -- then
            # the bytes must still be the reference's
            assert hashlib.sha256(out).hexdigest() == exp, f"allocation {k} failed and the output changed"
        except RuntimeError as e:
            failed += 1
            assert "memory" in str(e).lower() or "hip" in str(e).lower() or "failed" in str(e).lower(), str(e)
        finally:
            emu.gz_emu_fail_alloc(-1)
        assert live(emu) == base, f"allocation {k} of {total} failing leaves {live(emu)} behind"
    assert failed >= len(points) // 2, (failed, len(points))
    jpg, _ = host.process(rgb, quality=90.0)
    assert hashlib.sha256(jpg).hexdigest() == exp


# ---- launch failures: the context's claims on error paths (patch_reconstruct = 2: a Compare that trusts the linear
# planes checks them against a full reconstruction itself, so a stale claim is GZ_E_STATE there, not a quiet error)
TARGET = 0.971769
Q = np.full((3, 64), 3, np.int32)


@pytest.fixture(scope="module")
def L(emu):
    return Library(build_emu.build())


def compare_patched(L, ctx):
    """ctx.compare() and whether it relied on the patched planes / on the opsin image kept ahead."""
    before = L.compare_counters(all=True)
    got = ctx.compare()
    d = [a - b for a, b in zip(L.compare_counters(all=True), before)]
    return got, d[0] > 0, d[3] > 0


def assert_as_fresh(L, ctx, got, rgb):
    """got (ctx's Compare) bit for bit that of a fresh context given ctx's coefficients."""
    with L.context(rgb, TARGET) as fresh:
        fresh.set_coeffs(ctx.get_coeffs())
        exp = fresh.compare()
    for g, e, what in zip(got, exp, ("distance", "distance map", "block maxima")):
        assert_bits_equal(np.asarray(g, np.float32), np.asarray(e, np.float32), what)


def sweep_launches(emu, setup, call, after):
    """setup() -> state; call(state) once cleanly to count its launches, then for every launch n of it on a fresh
    state: launch n fails, the call fails with GZ_E_HIP, after(state, n) checks how the context goes on."""
    st = setup()
    before = emu.gz_emu_launch_calls()
    call(st)
    n_launches = emu.gz_emu_launch_calls() - before
    assert n_launches >= 1
    for n in range(n_launches):
        st = setup()
        emu.gz_emu_fail_launch(n)
        try:
            with pytest.raises(GuetzliAmdError, match="GZ_E_HIP"):
                call(st)
        finally:
            emu.gz_emu_fail_launch(-1)
        after(st, n)
    return n_launches


def patch_ready(L, rgb, search=True, **cfg):
    """A context in the search loop's steady state: the Compare's full reconstruction made lin[] the candidate's."""
    ctx = L.context(rgb, TARGET)
    ctx.set_config(patch_reconstruct=2, **cfg)
    ctx.encode_rgb(download=False)
    ctx.quantize(Q, download=False)
    cnt = None
    if search:
        cnt = np.diff(ctx.block_zeroing_orders()[0])
        ctx.order_reset()
    ctx.compare()
    if search:
        ctx.order_build_auto(1, 1, 1.0, True, np.zeros(ctx.nb, np.int32))
        ctx.jpeg_histograms(Q)
    return ctx, cnt


def steps_of(ctx, cnt):
    """Steps on fewer than half of the block positions (the patch path)."""
    sel = np.flatnonzero(cnt > 0)[: ctx.nb // 2 - 1].astype(np.int32)
    return sel, np.minimum(cnt[sel], 2).astype(np.int32)


def edits_of(ctx, n, seed):
    rng = np.random.default_rng(seed)
    pos = rng.choice(3 * ctx.nb * 64, size=n, replace=False).astype(np.int32)
    return pos, rng.integers(-40, 40, n).astype(np.int16)


def goes_on_unpatched(L, rgb):
    def after(ctx, n):
        got, patched, ahead = compare_patched(L, ctx)
        assert not patched and not ahead, f"launch {n} failed, and the next Compare trusted the patched planes"
        assert_as_fresh(L, ctx, got, rgb)
        ctx.close()
    return after


@pytest.mark.parametrize("ahead", [True, False])
def test_candidate_steps_launch_failures_drop_the_claims(emu, L, ahead):
    rgb = images.crop(40, 32, 100, 60)
    cfg = dict(single_stream=0, opsin_ahead=1) if ahead else dict(opsin_ahead=0)

    def call(st):
        ctx, cnt = st
        ctx.apply_candidate_steps(1, *steps_of(ctx, cnt))
    ctx, cnt = patch_ready(L, rgb, **cfg)
    call((ctx, cnt))
    _, patched, kept = compare_patched(L, ctx)
    assert patched and kept == ahead, "the clean call did not take the patch path"
    ctx.close()
    after = goes_on_unpatched(L, rgb)
    n = sweep_launches(emu, lambda: patch_ready(L, rgb, **cfg), call, lambda st, n: after(st[0], n))
    assert n >= (4 if ahead else 3), n


@pytest.mark.parametrize("ahead", [True, False])
def test_coeff_edits_launch_failures_drop_the_claims(emu, L, ahead):
    """The direct path (4096 edits or fewer), behind bulk steps that kept the opsin image ahead, or not."""
    rgb = images.crop(40, 32, 100, 60)
    cfg = dict(single_stream=0, opsin_ahead=1) if ahead else dict(opsin_ahead=0)

    def setup():
        ctx, cnt = patch_ready(L, rgb, **cfg)
        ctx.apply_candidate_steps(1, *steps_of(ctx, cnt))
        return ctx

    def call(ctx):
        ctx.apply_coeff_edits(*edits_of(ctx, 6, 7))
    ctx = setup()
    call(ctx)
    _, patched, kept = compare_patched(L, ctx)
    assert patched and kept == ahead, "the clean call did not take the patch path"
    ctx.close()
    n = sweep_launches(emu, setup, call, goes_on_unpatched(L, rgb))
    assert n >= (3 if ahead else 2), n


def test_bulk_coeff_edits_launch_failures_drop_the_claims(emu, L):
    """The bulk path (more than 4096 edits, through device memory) on an image with twice as many blocks."""
    rgb = images.tiled(1024, 520)   # 8320 blocks

    def setup():
        return patch_ready(L, rgb, search=False)[0]

    def call(ctx):
        ctx.apply_coeff_edits(*edits_of(ctx, 4100, 11))
    ctx = setup()
    call(ctx)
    assert compare_patched(L, ctx)[1], "the clean call did not take the patch path"
    ctx.close()
    assert sweep_launches(emu, setup, call, goes_on_unpatched(L, rgb)) >= 2


def test_quantize_launch_failure_drops_the_claims(emu, L):
    rgb = images.crop(40, 32, 100, 60)
    sweep_launches(emu, lambda: patch_ready(L, rgb, search=False)[0], lambda ctx: ctx.quantize(Q + 2),
                   goes_on_unpatched(L, rgb))


@pytest.mark.parametrize("planes", [False, True])
def test_downsample_launch_failures_leave_no_original(emu, L, planes):
    """A failed gz_downsample* leaves the 4:4:4 frame with a half-rewritten original: quantizing it is refused (the
    candidate and its planes are untouched: the next Compare may trust them -- and checks them itself)."""
    rgb = images.crop(40, 32, 100, 60)
    yuv = [np.ascontiguousarray(rgb[..., i], np.float32) for i in range(3)]

    def call(ctx):
        if planes:
            ctx.downsample_planes(*yuv, download=False)
        else:
            ctx.downsample(download=False)

    def after(ctx, n):
        got, _, _ = compare_patched(L, ctx)
        assert_as_fresh(L, ctx, got, rgb)
        co = ctx.get_coeffs()
        with pytest.raises(GuetzliAmdError, match="GZ_E_STATE"):
            ctx.quantize(Q)
        assert np.array_equal(ctx.get_coeffs(), co), f"launch {n} failed, and a half-written original was quantized"
        assert ctx.frame_layout()[0] == 1
        ctx.close()
    sweep_launches(emu, lambda: patch_ready(L, rgb, search=False)[0], call, after)


# ---- a failed call is repeated on the same context: every group the context makes on first use is all-or-nothing and
# counts as made only behind its initialisation (context.h, regrow), so the repeat finds nothing half-made
def _eq(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_eq(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


FIXED_CODES = (np.full((2, 3, 256), 8, np.uint8), np.tile(np.arange(256, dtype=np.uint16), (2, 3, 1)))   # 8 bits a symbol


def quantized(L, rgb):
    ctx = L.context(rgb, TARGET)
    ctx.encode_rgb(download=False)
    ctx.quantize(Q, download=False)
    return ctx


def searched(L, rgb):
    """... and phase A's block search, and a distance map (max_block_error is zeroed with the arrays it lives in)."""
    ctx = quantized(L, rgb)
    ctx.cnt = np.diff(ctx.block_zeroing_orders()[0])
    ctx.compare()
    return ctx


def zeros(ctx):
    return np.zeros(ctx.search_blocks, np.int32)


def ordered(L, rgb, histograms=False):
    ctx = searched(L, rgb)
    if histograms:
        ctx.jpeg_histograms(Q)
    ctx.total = ctx.order_build_auto(1, 1, 1.0, True, zeros(ctx))[0]
    return ctx


def scanned(L, rgb):
    ctx = quantized(L, rgb)
    ctx.jpeg_histograms(Q)
    ctx.jpeg_scan(3, *FIXED_CODES)
    return ctx


def _scan(ctx):
    return ctx.jpeg_scan(3, *FIXED_CODES), ctx.jpeg_scan_bytes()


def _scan_keep(ctx):
    ctx.jpeg_scan_keep()
    return ctx.jpeg_scan_bytes(kept=True)


def _compare_blocks(ctx):
    xy = np.array([[0, 0], [1, 1], [1, 0]], np.int32)
    co = ctx.get_coeffs()
    return ctx.compare_blocks(xy, np.stack([co[:, y * ctx.bw + x] for x, y in xy]))


def _fused(ctx):
    ctx.order_build_auto_descend_begin(1, 1, 1.0, True, zeros(ctx), 2.0, 16, 12)
    return ctx.order_build_auto_end(), ctx.order_descend_end(12)


def _steps(ctx):
    sel = np.flatnonzero(ctx.cnt > 0)[:1].astype(np.int32)   # one block of four: a minority, the patch path
    ctx.apply_candidate_steps(1, sel, np.minimum(ctx.cnt[sel], 2).astype(np.int32))
    return ctx.steps_histogram_delta(), ctx.get_coeffs()


def _edits(ctx):
    ctx.apply_coeff_edits(*edits_of(ctx, 6, 7))
    return ctx.get_coeffs()


def _mirror_fetch(ctx):
    return ctx.order_fetch(0, ctx.total, ctx.order_host_mirror(ctx.total)).copy()


# (name, the calls that bring a fresh context to the state the step needs, the step -> its results)
LAZY_STEPS = [
    ("gz_jpeg_histograms", quantized, lambda ctx: ctx.jpeg_histograms(Q)),
    ("gz_jpeg_scan", lambda L, rgb: (lambda ctx: (ctx.jpeg_histograms(Q), ctx)[1])(quantized(L, rgb)), _scan),
    ("gz_jpeg_scan_keep", scanned, _scan_keep),
    ("gz_block_zeroing_orders", quantized, lambda ctx: ctx.block_zeroing_orders()),
    ("gz_compare_blocks", quantized, _compare_blocks),
    ("gz_order_build_auto", searched, lambda ctx: (lambda r: (r, ctx.order_fetch(0, r[0])))(ctx.order_build_auto(1, 1, 1.0, True, zeros(ctx)))),
    ("gz_order_build_auto_descend_begin .. _end", searched, _fused),
    ("gz_order_descend", ordered, lambda ctx: (ctx.order_descend(ctx.total // 2, 16, 3), ctx.order_fetch(0, ctx.total))),
    ("gz_apply_candidate_steps + gz_steps_histogram_delta", lambda L, rgb: ordered(L, rgb, histograms=True), _steps),
    ("gz_apply_coeff_edits", quantized, _edits),
    ("gz_order_host_mirror + gz_order_fetch", ordered, _mirror_fetch),
]


def sweep_allocations(emu, L, rgb, name, setup, call, min_allocs=1):
    """call(setup()) once cleanly: its results, the distance of a Compare behind it, its allocations counted.  Then for
    EVERY allocation n of it, on a fresh context in the same state: allocation n fails -> GZ_E_NOMEM; the same call
    repeated on the same context -> the clean call's results, bit for bit; a Compare -> the clean context's distance;
    gz_destroy -> nothing left allocated."""
    base = live(emu)
    ctx = setup(L, rgb)
    before = emu.gz_emu_alloc_calls()
    exp = call(ctx)
    n_allocs = emu.gz_emu_alloc_calls() - before
    exp_dist = ctx.compare(want_distmap=False, want_block_max=False)[0]
    ctx.close()
    assert live(emu) == base, f"{name}: a clean call leaves allocations behind"
    assert n_allocs >= min_allocs, (name, n_allocs)
    for n in range(n_allocs):
        ctx = setup(L, rgb)
        emu.gz_emu_fail_alloc(n)
        try:
            with pytest.raises(GuetzliAmdError, match="GZ_E_NOMEM"):
                call(ctx)
        finally:
            emu.gz_emu_fail_alloc(-1)
        got = call(ctx)
        assert _eq(got, exp), f"{name}: repeated after allocation {n} of {n_allocs} failed, the call gives other results"
        assert bits_of(ctx.compare(want_distmap=False, want_block_max=False)[0]) == bits_of(exp_dist), (name, n)
        ctx.close()
        assert live(emu) == base, f"{name}: allocation {n} failing leaves {live(emu)} (device bytes, host bytes, blocks, events)"
    return n_allocs


def bits_of(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def test_a_context_survives_every_lazy_allocation_failing(emu, L):
    """The C ABI's caller may free memory and repeat a call that returned GZ_E_NOMEM.  Every allocation index of every
    step is swept (nothing sampled): 16x16 is four blocks and an order of 557 entries."""
    rgb = np.ascontiguousarray(images.crop(16, 16, 100, 60))
    counts = {name: sweep_allocations(emu, L, rgb, name, setup, call) for name, setup, call in LAZY_STEPS}
    # the groups made on first use are in there: the entropy coder's seven buffers and the landing area; the block mask,
    # the probe arena and the search's seven; the order's block arrays, its counters and its four growing buffers
    assert counts["gz_jpeg_histograms"] >= 8 and counts["gz_block_zeroing_orders"] >= 9, counts
    assert counts["gz_order_build_auto"] >= 14 and counts["gz_order_descend"] >= 3, counts
    # 4:2:0: the chroma samples (d_csamp) of the search with component mask 6, the 16x16 maxima (d_gmax) of its order
    rgb = np.ascontiguousarray(images.crop(32, 32, 100, 60))

    def downsampled(L, rgb):
        ctx = L.context(rgb, TARGET)
        ctx.encode_rgb(download=False)
        ctx.downsample(download=False)
        ctx.quantize(Q, download=False)
        return ctx

    def searched420(L, rgb):
        ctx = downsampled(L, rgb)
        ctx.block_zeroing_orders(comp_mask=6)
        ctx.compare()
        return ctx
    n = sweep_allocations(emu, L, rgb, "4:2:0 gz_block_zeroing_orders_masked(6)", downsampled,
                          lambda ctx: ctx.block_zeroing_orders(comp_mask=6))
    assert n >= 10, n
    n = sweep_allocations(emu, L, rgb, "4:2:0 gz_order_build_auto", searched420,
                          lambda ctx: ctx.order_build_auto(1, 1, 1.0, True, zeros(ctx)))
    assert n >= 15, n


def test_initialisation_failures_leave_the_group_unmade(emu, L):
    """A group's memset or table upload fails to enqueue: the call fails, and the repeat makes the group again -- its
    results are the clean call's bit for bit (the emulation poisons fresh memory with 0xCD: a group that counted as made
    without its initialisation shows in max_block_error, the ranking tables or the scan's look-back flags)."""
    emu.gz_emu_fail_copy.argtypes = [C.c_long]
    emu.gz_emu_copy_calls.restype = C.c_long
    rgb = np.ascontiguousarray(images.crop(16, 16, 100, 60))
    first_scan = LAZY_STEPS[1]
    for name, setup, call in (LAZY_STEPS[5], LAZY_STEPS[3], first_scan):
        ctx = setup(L, rgb)
        before = emu.gz_emu_copy_calls()
        exp = call(ctx)
        n_copies = emu.gz_emu_copy_calls() - before
        ctx.close()
        assert n_copies >= 3, (name, n_copies)
        for n in range(n_copies):   # (every asynchronous copy and fill of the call, the group's initialisation among them)
            ctx = setup(L, rgb)
            emu.gz_emu_fail_copy(n)
            try:
                with pytest.raises(GuetzliAmdError, match="GZ_E_HIP"):
                    call(ctx)
            finally:
                emu.gz_emu_fail_copy(-1)
            assert _eq(call(ctx), exp), f"{name}: repeated after copy {n} of {n_copies} failed, the call gives other results"
            ctx.close()
