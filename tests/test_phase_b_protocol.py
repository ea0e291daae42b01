"""The protocol of phase B's two-phase calls (entry_phaseb.h, entry_compare.h): what is in flight between a _begin and
its _end, in which order the ends may come, what voids a pending call, and what a voided call's _end returns.

A table of rows.  Each row is a call sequence on a fresh context and its outcome: return codes, and results compared
bit for bit with the synchronous forms (gz_order_build_auto, gz_order_descend, gz_compare) on another fresh context
given the same candidate -- no constant is recorded.  The rows run one by one over the CPU emulation, and once more as
one test on the device.  The launch-failure rows need the emulation's failing launches and run there only.

Rows marked `# parent behaviour, suspect` pinned what the entries did, before the pending state had one owner
(context.h, struct Pending), where that contradicted context.h's rule -- a voided call's _end returns nothing.  They
say what that was, and assert what the rule asks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import fields
from guetzli_amd.capi import GuetzliAmdError, Library

W, H = 100, 84
TARGET = 0.971769
Q = np.full((3, 64), 3, np.int32)
PER_BLOCK, THRESHOLD, LEVELS = 2.0, 16, 12
STATE, HIP = "GZ_E_STATE", "GZ_E_HIP"


@pytest.fixture(scope="module")
def emu():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
    import build_emu
    L = Library(build_emu.build())
    L.lib.gz_emu_fail_launch.argtypes = [C.c_long]
    L.lib.gz_emu_launch_calls.restype = C.c_long
    return L


def searched(L):
    """A fresh context as phase B finds it: a candidate, phase A's block search, max_block_error zeroed, a distance map."""
    ctx = L.context(fields.primaries(W, H), TARGET)
    ctx.encode_rgb(download=False)
    ctx.quantize(Q, download=False)
    off, _, _ = ctx.block_zeroing_orders()
    ctx.order_reset()
    ctx.compare()
    ctx.cnt = np.diff(off)
    return ctx


def next_cands(ctx):
    """Two states of the search: no block has advanced; every block with two candidates or more has taken one."""
    return np.zeros(ctx.nb, np.int32), (ctx.cnt > 1).astype(np.int32)


def derived_last(total, btc):
    """The position the device derives for the descent (gz_kernels_order.h, desc_load; processor.cc:685-687, :739-741)."""
    min_coeffs = max(0, int(np.float32(PER_BLOCK) * np.float32(btc)))
    fast_until = min(min_coeffs, total - 1) // 10 * 10
    return fast_until - 1 if fast_until else 0


def bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


class Reference:
    """The synchronous forms on fresh contexts given the same candidate, one per state of next_cand; made once."""

    def __init__(self, L):
        self.results, self.cuts, self.last, self.entries = [], [], [], []
        for i in range(2):
            with searched(L) as ctx:
                if i == 0:
                    self.distance = bits(ctx.compare(want_distmap=False, want_block_max=False)[0])
                total, btc, below = ctx.order_build_auto(1, 1, 1.0, True, next_cands(ctx)[i])
                last = derived_last(total, btc)
                cuts = ctx.order_descend(last, THRESHOLD, LEVELS)
                assert total > THRESHOLD and btc > 0 and len(cuts) >= 1, "a reference that exercises nothing"
                self.results.append((total, btc, below))
                self.cuts.append(cuts)
                self.last.append(last)
                self.entries.append(ctx.order_fetch(0, total))
        assert self.results[0] != self.results[1], "the two states of next_cand give one order"


def fused_begin(ctx, which=0, levels=LEVELS):
    ctx.order_build_auto_descend_begin(1, 1, 1.0, True, next_cands(ctx)[which], PER_BLOCK, THRESHOLD, levels)


def split_begin(ctx, which=0):
    ctx.order_build_auto_begin(1, 1, 1.0, True, next_cands(ctx)[which])


def fails(call, code, text=None):
    with pytest.raises(GuetzliAmdError, match=code) as e:
        call()
    if text:
        assert text in str(e.value), str(e.value)


def order_is(ctx, ref, which=0):
    assert ctx.order_build_auto_end() == ref.results[which]


def descent_is(ctx, ref, which=0):
    cuts, last = ctx.order_descend_end(LEVELS)
    assert np.array_equal(cuts, ref.cuts[which]) and last == ref.last[which], (cuts, last)


def no_order(ctx):
    fails(ctx.order_build_auto_end, STATE, "gz_order_build_auto_begin must precede gz_order_build_auto_end")


def no_descent(ctx):
    cuts, last = ctx.order_descend_end(LEVELS)
    assert len(cuts) == 0 and last == 0


def distance_is(ctx, ref):
    assert bits(ctx.compare_end()) == ref.distance


def no_compare(ctx):
    fails(ctx.compare_end, STATE, "gz_compare_begin must precede gz_compare_end")


def nothing_pending(ctx):
    no_order(ctx)
    no_descent(ctx)
    no_compare(ctx)
    ctx.set_config(single_stream=ctx.get_config().single_stream)   # (accepted: nothing is in flight)


# ---- the rows: function(L, ref)
def row_ends_without_begins(L, ref):
    with searched(L) as ctx:
        no_order(ctx)
        no_descent(ctx)
        assert ctx.order_exported() == 0
        fails(lambda: ctx.order_descend_begin(PER_BLOCK, THRESHOLD, LEVELS), STATE,
              "gz_order_build_auto_begin must precede gz_order_descend_begin")
        no_compare(ctx)


def row_order_of_ends(L, ref):
    with searched(L) as ctx:
        mirror = ctx.order_host_mirror(int(ctx.cnt.sum()))
        fused_begin(ctx)
        fails(lambda: ctx.order_descend_end(LEVELS), STATE, "gz_order_build_auto_end must precede gz_order_descend_end")
        fails(ctx.order_exported, STATE, "gz_order_descend_end must precede gz_order_exported")
        order_is(ctx, ref)
        fails(ctx.order_exported, STATE, "gz_order_descend_end must precede gz_order_exported")
        descent_is(ctx, ref)
        n = ctx.order_exported()
        assert 0 < n <= ref.results[0][0]
        assert np.array_equal(mirror[:n], ref.entries[0][:n]), "the exported prefix is not the synchronous descent's"
        assert ctx.order_exported() == n   # (no end: it may be asked again)


def row_order_of_ends_split(L, ref):
    with searched(L) as ctx:
        split_begin(ctx)
        ctx.order_descend_begin(PER_BLOCK, THRESHOLD, LEVELS)
        fails(lambda: ctx.order_descend_end(LEVELS), STATE, "gz_order_build_auto_end must precede gz_order_descend_end")
        fails(ctx.order_exported, STATE)
        order_is(ctx, ref)
        descent_is(ctx, ref)
        assert ctx.order_exported() == 0   # (only the fused call exports)


def row_second_end(L, ref):
    with searched(L) as ctx:
        ctx.compare_begin()
        fused_begin(ctx)
        distance_is(ctx, ref)
        order_is(ctx, ref)
        descent_is(ctx, ref)
        no_compare(ctx)
        no_order(ctx)
        no_descent(ctx)   # (gz_order_descend_end has no state error of its own: a second one returns nothing)


def row_fused_compare_end_first(L, ref):
    with searched(L) as ctx:
        ctx.compare_begin()
        fused_begin(ctx)
        distance_is(ctx, ref)
        order_is(ctx, ref)
        descent_is(ctx, ref)
        assert np.array_equal(ctx.order_fetch(0, ref.results[0][0]), ref.entries[0])


def row_fused_compare_end_last(L, ref):
    with searched(L) as ctx:
        ctx.compare_begin()
        fused_begin(ctx)
        order_is(ctx, ref)
        descent_is(ctx, ref)
        distance_is(ctx, ref)
        assert np.array_equal(ctx.order_fetch(0, ref.results[0][0]), ref.entries[0])


def row_fused_superseded_by_fused(L, ref):
    """The second begin's results are the ones every end returns; one end each."""
    with searched(L) as ctx:
        ctx.compare_begin()
        fused_begin(ctx, 0)
        fused_begin(ctx, 1)
        order_is(ctx, ref, 1)
        descent_is(ctx, ref, 1)
        distance_is(ctx, ref)
        nothing_pending(ctx)


def row_fused_superseded_by_synchronous(L, ref):
    """gz_order_build_auto voids the pending order and its descent; the Compare's distance still arrives."""
    with searched(L) as ctx:
        ctx.compare_begin()
        fused_begin(ctx, 0)
        assert ctx.order_build_auto(1, 1, 1.0, True, next_cands(ctx)[1]) == ref.results[1]
        no_order(ctx)
        no_descent(ctx)
        distance_is(ctx, ref)
        assert np.array_equal(ctx.order_descend(ref.last[1], THRESHOLD, LEVELS), ref.cuts[1])


def row_split_superseded_by_fused(L, ref):
    with searched(L) as ctx:
        split_begin(ctx, 0)
        ctx.order_descend_begin(PER_BLOCK, THRESHOLD, LEVELS)
        fused_begin(ctx, 1)
        order_is(ctx, ref, 1)
        descent_is(ctx, ref, 1)
        nothing_pending(ctx)


def new_frame(how):
    def row(L, ref):
        with searched(L) as ctx:
            ctx.order_host_mirror(int(ctx.cnt.sum()))
            ctx.compare_begin()
            fused_begin(ctx)
            if how == "set_frame":
                ctx.set_frame(2)
            else:
                ctx.downsample(download=False)
            no_order(ctx)
            no_descent(ctx)
            no_compare(ctx)
            assert ctx.order_exported() == 0
    return row


def row_set_config_while_pending(L, ref):
    busy = "gz_set_config while work of the context is in flight"
    with searched(L) as ctx:
        again = lambda: ctx.set_config(single_stream=ctx.get_config().single_stream)   # noqa: E731
        again()
        ctx.compare_begin()
        fails(again, STATE, busy)
        fused_begin(ctx)
        fails(again, STATE, busy)
        distance_is(ctx, ref)
        fails(again, STATE, busy)   # (the order and the descent)
        order_is(ctx, ref)
        fails(again, STATE, busy)   # (the descent)
        descent_is(ctx, ref)
        again()
        split_begin(ctx)
        fails(again, STATE, busy)
        order_is(ctx, ref)
        again()


def replaced_order(how):
    def row(L, ref):
        with searched(L) as ctx:
            ctx.compare_begin()
            fused_begin(ctx)
            if how == "upload":
                ctx.order_upload(ref.entries[1])
            elif how == "build":
                nb = ctx.nb
                ctx.order_build(1, next_cands(ctx)[1], np.zeros(nb, np.float32), np.ones(nb, np.float32))
            else:
                ctx.block_zeroing_orders()
            no_order(ctx)
            # parent behaviour, suspect: gz_order_upload, gz_order_build and gz_block_zeroing_orders voided the pending
            # order but not the descent enqueued behind it, and this gz_order_descend_end handed out the cut log and
            # `last` of the order that had been replaced -- descent_is(ctx, ref, 0).  Now a voided call's _end returns
            # nothing.
            no_descent(ctx)
            distance_is(ctx, ref)   # (the evaluation is not the order's: its distance still arrives)
    return row


def failed_begin(fused):
    """Every launch of the _begin fails in turn, with a Compare pending: nothing of the call stays pending, the
    Compare's distance arrives, and a clean repeat gives the clean results.  Emulation only.
    (The fused call with one level more than the descent takes: the launches of further idle levels are the same.)"""
    def row(L, ref):
        from test_hip_failures import sweep_launches
        levels = len(ref.cuts[0]) + 1

        def begin(ctx):
            if fused:
                fused_begin(ctx, 0, levels)
            else:
                split_begin(ctx)

        def setup():
            ctx = searched(L)
            ctx.order_host_mirror(int(ctx.cnt.sum()))
            ctx.compare_begin()
            return ctx

        def after(ctx, n):
            no_order(ctx)
            no_descent(ctx)
            assert ctx.order_exported() == 0
            distance_is(ctx, ref)
            ctx.compare_begin()
            begin(ctx)
            distance_is(ctx, ref)
            order_is(ctx, ref)
            if fused:
                descent_is(ctx, ref)
            else:
                no_descent(ctx)
            ctx.close()
        n = sweep_launches(L.lib, setup, begin, after)
        # the weights' two kernels and the fill; the fused call: two launches per level of the descent and the export
        assert n == (3 + 2 * levels + 1 if fused else 3), n
    return row


ROWS = {
    "ends_without_begins": row_ends_without_begins,
    "order_of_ends": row_order_of_ends,
    "order_of_ends_split": row_order_of_ends_split,
    "second_end": row_second_end,
    "fused_compare_end_first": row_fused_compare_end_first,
    "fused_compare_end_last": row_fused_compare_end_last,
    "fused_superseded_by_fused": row_fused_superseded_by_fused,
    "fused_superseded_by_synchronous": row_fused_superseded_by_synchronous,
    "split_superseded_by_fused": row_split_superseded_by_fused,
    "set_frame_between_begin_and_end": new_frame("set_frame"),
    "downsample_between_begin_and_end": new_frame("downsample"),
    "set_config_while_pending": row_set_config_while_pending,
    "order_upload_after_fused_begin": replaced_order("upload"),
    "order_build_after_fused_begin": replaced_order("build"),
    "block_search_after_fused_begin": replaced_order("search"),
}
EMU_ROWS = {
    "fused_begin_launch_failures": failed_begin(True),
    "split_begin_launch_failures": failed_begin(False),
}


@pytest.fixture(scope="module")
def emu_ref(emu):
    return Reference(emu)


@pytest.mark.parametrize("name", list(ROWS) + list(EMU_ROWS))
def test_protocol_row(emu, emu_ref, name):
    (ROWS.get(name) or EMU_ROWS[name])(emu, emu_ref)


@pytest.mark.gpu
def test_protocol_table_on_the_device():
    import guetzli_amd
    L = guetzli_amd.load()
    ref = Reference(L)
    for name, row in ROWS.items():
        try:
            row(L, ref)
        except BaseException as e:
            raise AssertionError(f"row {name}: {e}") from e
