"""What the host code enqueues, where and in which order: kernel launches (name, grid, block, stream), event records
and waits, asynchronous copies and fills, synchronisations -- as the CPU emulation's opt-in enqueue log
(tests/emu/hip_emu.h) lists them, against recordings under tests/golden/enqueue_order/.

The emulation runs every launch at once on one thread, and on the device a missing wait between two streams is a race
that usually still gives the right bits: no other test sees the fork / join graph of the three-stream Compare chain, of
the next_cand upload beside it, or of the patches behind the step statistics.  The recordings pin it; a change that
is not meant to move work between streams or reorder it leaves them as they are.  Recording anew:
`python tests/test_enqueue_order.py` (only for a change that is meant to alter the order).
CPU only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "emu"), os.path.dirname(HERE)]   # (the second: run as a script, to record)
import build_emu  # noqa: E402
import fields  # noqa: E402
import parity_cases as pc  # noqa: E402
from guetzli_amd.capi import Library  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "enqueue_order")
W, H = 100, 84        # two tile columns, the second partial; 84 rows: a partial last tile row at 16 and at 32 rows
TARGET = 0.971769
Q = np.full((3, 64), 3, np.int32)


def load_library():
    lib = Library(build_emu.build())
    lib.lib.gz_emu_enqueue_log_fetch.restype = C.c_long
    lib.lib.gz_emu_enqueue_log_fetch.argtypes = [C.c_char_p, C.c_long]
    return lib


@pytest.fixture(scope="module")
def L():
    return load_library()


class Log:
    """with Log(L) as log: ... -> log.text"""

    def __init__(self, L):
        self.lib = L.lib

    def __enter__(self):
        self.lib.gz_emu_enqueue_log_start()
        return self

    def __exit__(self, *a):
        self.lib.gz_emu_enqueue_log_stop()
        n = self.lib.gz_emu_enqueue_log_fetch(None, 0)
        buf = C.create_string_buffer(n + 1)
        self.lib.gz_emu_enqueue_log_fetch(buf, n)
        self.text = buf.raw[:n].decode()


def rgb():
    return fields.primaries(W, H)


def candidate(L, **config):
    """A fresh context with a candidate in place."""
    ctx = L.context(rgb(), TARGET)
    ctx.set_config(**config)
    ctx.encode_rgb(download=False)
    ctx.quantize(Q, download=False)
    return ctx


# ---- the scenarios: name -> function(L) that returns the log's text
def create_and_set_rgb(L):
    with Log(L) as log:
        with L.context(rgb(), TARGET) as ctx:
            ctx.set_rgb(rgb())
    return log.text


def compare(single_stream, distmap, **config):
    def run(L):
        with candidate(L, single_stream=single_stream, **config) as ctx:
            with Log(L) as log:
                ctx.compare(want_distmap=distmap)
        return log.text
    return run


def patched(single_stream):
    """A phase-B iteration as the search loop drives it, with gz_config.patch_reconstruct = 2 (every Compare that
    trusts the patched planes checks them itself): bulk steps on a third of the blocks with the patches behind the
    statistics event and (three streams) the opsin blur ahead, two serial edits that cost a list of opsin tiles,
    gz_compare_begin, the next order with its next_cand upload beside the chain, gz_compare_end."""
    def run(L):
        with candidate(L, single_stream=single_stream, patch_reconstruct=2, opsin_ahead=1) as ctx:
            off, _, _ = ctx.block_zeroing_orders()
            nb = ctx.nb
            ctx.order_reset()
            ctx.compare()   # (the full reconstruction: the planes are the candidate's)
            next_cand = np.zeros(nb, np.int32)
            before = L.compare_counters(all=True)
            with Log(L) as log:
                ctx.order_build_auto(1, 1, 1.0, True, next_cand)
                ctx.jpeg_histograms(Q)
                sel = np.flatnonzero((np.arange(nb) % 3 == 0) & (np.diff(off) > 0)).astype(np.int32)
                ctx.apply_candidate_steps(1, sel, np.ones(sel.size, np.int32))
                ctx.steps_histogram_delta()
                next_cand[sel] += 1
                # blocks (2, 0) and (10, 0): one opsin tile each, in different tile columns
                pos = np.array([2 * 64 + 5, 10 * 64 + 9], np.int32)
                ctx.apply_coeff_edits(pos, np.array([7, -7], np.int16))
                ctx.compare_begin()
                ctx.order_build_auto_begin(1, 1, 1.0, True, next_cand)
                ctx.compare_end()
                ctx.order_build_auto_end()
            patched_, checked, compares, ahead, ahead_checked = (a - b for a, b in zip(L.compare_counters(all=True), before))
            assert 0 < 2 * sel.size <= nb
            assert (patched_, checked, compares) == (1, 1, 1)
            assert ahead == ahead_checked == (0 if single_stream else 1)
        return log.text
    return run


# ---- phase B's order protocol (entry_phaseb.h): the synchronous, the split and the fused form
PER_BLOCK, THRESHOLD, LEVELS = 2.0, 16, 12   # the descent's derivation of `last`, its floor, the log's capacity


def searched(L, **config):
    """A candidate with phase A's block search made, max_block_error zeroed and a distance map in place."""
    ctx = candidate(L, **config)
    off, _, _ = ctx.block_zeroing_orders()
    ctx.order_reset()
    ctx.compare()
    return ctx, off


def launches(text, kernel):
    return sum(ln.startswith("launch %s " % kernel) for ln in text.splitlines())


def phase_b_fused(single_stream):
    """The search loop's iteration: the next order and its descent enqueued behind the evaluation in flight as ONE
    call, whose results and the Compare's distance arrive in the descent's state; gz_order_advance's update then rides
    on the next order's k_weights_gather."""
    def run(L):
        ctx, off = searched(L, single_stream=single_stream)
        with ctx:
            next_cand = np.zeros(ctx.nb, np.int32)
            with Log(L) as log:
                ctx.order_host_mirror(int(off[-1]))
                ctx.compare_begin()
                ctx.order_build_auto_descend_begin(1, 1, 1.0, True, next_cand, PER_BLOCK, THRESHOLD, LEVELS)
                ctx.compare_end()
                total, btc, _ = ctx.order_build_auto_end()
                cuts, last = ctx.order_descend_end(LEVELS)
                exported = ctx.order_exported()
                ctx.order_advance(0.25, 1)
                ctx.compare_begin()
                ctx.order_build_auto_descend_begin(1, 1, 1.0, True, next_cand, PER_BLOCK, THRESHOLD, LEVELS)
                ctx.compare_end()
                total2, _, _ = ctx.order_build_auto_end()
                cuts2, _ = ctx.order_descend_end(LEVELS)
            assert total > THRESHOLD and btc > 0 and len(cuts) >= 1 and 0 < last < total
            assert 0 < exported <= total, "k_desc_export wrote no prefix into the host mirror"
            assert total2 > 0 and len(cuts2) >= 1
            assert launches(log.text, "k_desc_export") == 2
            assert launches(log.text, "k_order_advance") == 0, "the advance was to ride on k_weights_gather"
        return log.text
    return run


def phase_b_split(L):
    """gz_order_build_auto_begin, gz_order_descend_begin behind it, the ends; two advances in a row."""
    ctx, _ = searched(L, single_stream=0)
    with ctx:
        next_cand = np.zeros(ctx.nb, np.int32)
        with Log(L) as log:
            ctx.order_build_auto_begin(1, 1, 1.0, True, next_cand)
            ctx.order_descend_begin(PER_BLOCK, THRESHOLD, LEVELS)
            total, btc, _ = ctx.order_build_auto_end()
            cuts, last = ctx.order_descend_end(LEVELS)
            ctx.order_advance(0.25, 1)
            ctx.order_advance(0.5, 1)
        assert total > THRESHOLD and btc > 0 and len(cuts) >= 1 and 0 < last < total
        assert launches(log.text, "k_desc_export") == 0
        assert launches(log.text, "k_order_advance") == 1, "the first of two advances is made by a launch of its own"
    return log.text


def phase_b_sync(L):
    """The order from the caller's arrays, the descent and one partition in one call each, the fetches' three paths
    (into the pinned mirror, through the landing area into pageable memory, an empty range), an upload."""
    ctx, off = searched(L, single_stream=0)
    with ctx:
        nb = ctx.nb
        with Log(L) as log:
            total, btc, _ = ctx.order_build(1, np.zeros(nb, np.int32), np.zeros(nb, np.float32),
                                            np.ones(nb, np.float32))
            cuts = ctx.order_descend(total // 4, THRESHOLD, LEVELS)
            cut = ctx.order_partition(0, total)
            mirror = ctx.order_host_mirror(total)
            ctx.order_fetch(0, total, out=mirror)
            entries = ctx.order_fetch(0, total)
            ctx.order_fetch(total, total)
            ctx.order_upload(entries)
        assert total == int(off[-1]) and btc > 0 and len(cuts) >= 1 and 0 < cut <= total
        assert np.array_equal(mirror, entries)
        assert launches(log.text, "k_order_sizes") == 1 and launches(log.text, "k_part_swap") == 1
    return log.text


def bulk_steps_without_statistics(L):
    """gz_apply_candidate_steps before any gz_jpeg_histograms: k_apply_steps, no symbol statistics."""
    ctx, off = searched(L, single_stream=0)
    with ctx:
        nb = ctx.nb
        ctx.order_build_auto(1, 1, 1.0, True, np.zeros(nb, np.int32))
        sel = np.flatnonzero((np.arange(nb) % 3 == 0) & (np.diff(off) > 0)).astype(np.int32)
        with Log(L) as log:
            ctx.apply_candidate_steps(1, sel, np.ones(sel.size, np.int32))
        assert sel.size > 0
        assert launches(log.text, "k_apply_steps") == 1 and launches(log.text, "k_apply_steps_hist") == 0
    return log.text


def bulk_edits(L):
    """gz_apply_coeff_edits with more than 4096 positions: through device memory, not the staging buffer."""
    with candidate(L, single_stream=0) as ctx:
        n = 4100
        assert n <= 3 * ctx.nb * 64
        pos = (np.arange(n, dtype=np.int64) * 6 + 1).astype(np.int32)   # distinct, spread over all three components
        assert pos[-1] < 3 * ctx.nb * 64
        with Log(L) as log:
            ctx.apply_coeff_edits(pos, np.full(n, 3, np.int16))
        assert launches(log.text, "k_apply_coeff_edits") == 1
        assert sum(ln.startswith("memcpy h2d ") for ln in log.text.splitlines()) == 2, "the device-memory arm"
    return log.text


def compare_420(L):
    with L.context(rgb(), TARGET) as ctx:
        ctx.set_config(single_stream=0)
        ctx.encode_rgb(download=False)
        ctx.downsample(download=False)
        ctx.quantize(Q, download=False)
        with Log(L) as log:
            ctx.compare()
    return log.text


def block_zeroing_orders(L):
    with candidate(L) as ctx:
        with Log(L) as log:
            ctx.block_zeroing_orders()
    return log.text


def probes(L):
    img = rgb()
    lin0 = fields.linear(img)
    lin1 = np.ascontiguousarray(np.roll(lin0, 1, axis=2))
    with L.context(img, TARGET) as ctx:
        ctx.set_config(single_stream=0)
        with Log(L) as log:
            ctx.probe_mask(lin0, lin1)
            ctx.probe_diffmap(lin0, lin1)
            ctx.probe_blur(lin0[0], *pc.SIGMAS_BR[6])   # radius 5: one fused launch
            ctx.probe_blur(lin0[0], *pc.SIGMAS_BR[5])   # radius 20: a row and a column pass
    return log.text


SCENARIOS = {
    "create_and_set_rgb": create_and_set_rgb,
    "compare_three_streams": compare(0, False),
    "compare_three_streams_distmap": compare(0, True),
    "compare_one_stream": compare(1, False),
    "compare_one_stream_distmap": compare(1, True),
    "patched_three_streams": patched(0),
    "patched_one_stream": patched(1),
    "phase_b_fused_three_streams": phase_b_fused(0),
    "phase_b_fused_one_stream": phase_b_fused(1),
    "phase_b_split": phase_b_split,
    "phase_b_sync": phase_b_sync,
    "bulk_steps_without_statistics": bulk_steps_without_statistics,
    "bulk_edits": bulk_edits,
    "compare_420": compare_420,
    "block_zeroing_orders": block_zeroing_orders,
    "probes": probes,
}
for _cfg in pc.ALL_INSTANTIATIONS:
    SCENARIOS["compare_packed%d_rows%d" % (_cfg["blur_packed"], _cfg["tile_rows"])] = compare(0, False, **_cfg)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_enqueue_order(L, name):
    got = SCENARIOS[name](L)
    with open(os.path.join(GOLDEN, name + ".txt")) as f:
        exp = f.read()
    assert got.splitlines() == exp.splitlines()


@pytest.mark.parametrize("distmap", [False, True])
def test_one_stream_chain_has_no_fork_or_join(L, distmap):
    lines = compare(1, distmap)(L).splitlines()
    launches = [i for i, ln in enumerate(lines) if ln.startswith("launch ")]
    assert len(launches) >= 15, lines
    chain = lines[launches[0]:launches[-1] + 1]
    assert not [ln for ln in chain if ln.startswith(("record ", "wait "))], chain
    assert len({ln.split()[-1] for ln in chain}) == 1, "every call of the chain names the one stream"


def test_three_stream_chain_uses_three_streams(L):
    lines = compare(0, False)(L).splitlines()
    assert len({ln.split()[-1] for ln in lines if ln.startswith("launch ")}) == 3


if __name__ == "__main__":
    lib = load_library()
    os.makedirs(GOLDEN, exist_ok=True)
    for name_, run_ in sorted(SCENARIOS.items()):
        text = run_(lib)
        with open(os.path.join(GOLDEN, name_ + ".txt"), "w") as f:
            f.write(text)
        print(name_, len(text.splitlines()), "lines")
