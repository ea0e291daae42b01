"""gz_butteraugli_batch (and guetzli_amd.butteraugli_batch above it) without a GPU: the batched kernels through the CPU
emulation, where "device memory" is host memory; the argument checks, which come before any device call; the enqueue
log; every launch and allocation failing in turn; the batched kernels' bounds under the host sanitizers.  The cases
shared with the GPU suite are in tests/butteraugli_batch_cases.py.  CPU only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(HERE, "emu")]
import build_emu  # noqa: E402
import butteraugli_batch_cases as bbc  # noqa: E402
import butteraugli_pair_cases as bpc  # noqa: E402
from checkers import oracle, ref  # noqa: E402
from guetzli_amd import capi  # noqa: E402
from guetzli_amd.capi import Library, device_batch, device_map_batch  # noqa: E402

needs_ref = pytest.mark.skipif(ref is None, reason="oracle/_ref/libgz_ref.so not built")
CHECKERS = [pytest.param(oracle, id="oracle"), pytest.param(ref, id="ref", marks=needs_ref)]
MEM = bpc.HostMemory()
PRODUCER, CONSUMER = 0x5EED0, 0x5EED8   # stream handles of the caller's: the emulation only names them
W, H, N = 67, 33, 3


@pytest.fixture(scope="module")
def L():
    lib = Library(build_emu.build())
    lib.lib.gz_emu_enqueue_log_fetch.restype = C.c_long
    lib.lib.gz_emu_enqueue_log_fetch.argtypes = [C.c_char_p, C.c_long]
    lib.lib.gz_emu_fail_alloc.argtypes = [C.c_long]
    lib.lib.gz_emu_alloc_calls.restype = C.c_long
    lib.lib.gz_emu_live.argtypes = [C.POINTER(C.c_long)] * 4
    lib.lib.gz_emu_fail_launch.argtypes = [C.c_long]
    lib.lib.gz_emu_launch_calls.restype = C.c_long
    return lib


class enqueue_log:
    """with enqueue_log(L) as log: ... -> log.text, the emulation's enqueue log (tests/test_enqueue_order.py)."""

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


def live(lib):
    v = [C.c_long() for _ in range(4)]
    lib.gz_emu_live(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)   # device bytes, page-locked bytes, blocks, events


# ------------------------------------------------------------------ the cases shared with the GPU suite ----
@pytest.mark.parametrize("chk", CHECKERS)
@pytest.mark.parametrize("shape", bbc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_parity_at_every_shape(L, chk, shape):
    bbc.case_parity(L, MEM, chk, shape[0], shape[1], 3)


@pytest.mark.parametrize("chk", CHECKERS)
@pytest.mark.parametrize("n", bbc.BATCH_SIZES)
def test_parity_at_every_batch_size(L, chk, n):
    bbc.case_parity(L, MEM, chk, W, H, n)


@pytest.mark.parametrize("chk", CHECKERS)
@pytest.mark.parametrize("shape", bbc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_reference_for_all(L, chk, shape):
    bbc.case_broadcast(L, MEM, chk, shape[0], shape[1], 3)


@pytest.mark.parametrize("layout", bbc.IN_LAYOUTS)
@pytest.mark.parametrize("dtype", bbc.DTYPES)
def test_every_way_in(L, dtype, layout):
    bbc.case_way_in(L, MEM, ref or oracle, dtype, layout)


@pytest.mark.parametrize("layout", bbc.MAP_LAYOUTS)
@pytest.mark.parametrize("dtype", bpc.MAP_DTYPES)
def test_maps_of_every_type_and_layout(L, dtype, layout):
    bbc.case_maps(L, MEM, ref or oracle, dtype, layout)


def batched_chain_launches(L, n, n_ref, maps, scratch_bytes=0):
    """The launches of one call, counted by the emulation."""
    refs, others = bbc.pairs(W, H, n)
    before = L.lib.gz_emu_launch_calls()
    bbc.run_batch(L, MEM, bbc.lay_out(refs[:n_ref], "uint8", "NHWC"), bbc.lay_out(others, "uint8", "NHWC"), W, H, n, n_ref=n_ref,
                  maps=bbc.MapBatchDestination(n, W, H, "float32", "contiguous") if maps else None, scratch_bytes=scratch_bytes)
    return L.lib.gz_emu_launch_calls() - before


def test_chunks_of_two_give_the_unchunked_bits(L):
    bbc.case_chunking(L, MEM)
    # the chunk count, through the launch counter: a chunk of distinct references is one reference pass (9 launches), the
    # distorted images' (8), the difference's 9 and the emit; 5 images under a cap of 2 are 3 chunks
    per_chunk = batched_chain_launches(L, 2, 2, True)
    assert per_chunk == batched_chain_launches(L, 5, 5, True) == batched_chain_launches(L, 1, 1, True), "no launch per image"
    assert batched_chain_launches(L, 5, 5, True, scratch_bytes=2 * bbc.arena_bytes(W, H) + 64) == 3 * per_chunk
    assert batched_chain_launches(L, 5, 5, True, scratch_bytes=1) == 5 * per_chunk   # (a chunk is one image at the least)
    # one reference for all: a lone image's reference pass has the launches of a batched one, and it runs once, not per
    # chunk -- three chunks are one reference pass R and three distorted halves D, where a chunk of pairs is R + D
    assert batched_chain_launches(L, 5, 1, True) == per_chunk
    three = batched_chain_launches(L, 5, 1, True, scratch_bytes=2 * bbc.arena_bytes(W, H) + 64)
    reference_pass = (3 * per_chunk - three) // 2
    assert three < 3 * per_chunk and (3 * per_chunk - three) % 2 == 0 and 8 <= reference_pass < per_chunk / 2, (per_chunk, three)


# ------------------------------------------------------------------ the enqueue log ----
def test_the_enqueue_order(L):
    """The producers' streams are waited for in front of the first ingest kernel; the consumer's stream of the maps is
    waited for in front of the emit kernel and waits behind it; ONE stream carries the chain; the call ends with its own
    synchronise; the launches do not grow with the batch."""
    texts = {}
    for n in (2, 5):
        refs, others = bbc.pairs(W, H, n)
        rb, r_held = bbc.lay_out(refs, "uint8", "NHWC").on(MEM, PRODUCER)
        ob, o_held = bbc.lay_out(others, "uint8", "NHWC").on(MEM, PRODUCER)
        mb, m_held = bbc.MapBatchDestination(n, W, H, "float32", "contiguous").on(MEM, CONSUMER)
        dist = np.zeros(n, np.float32)
        with enqueue_log(L) as log:
            L.butteraugli_batch(rb, ob, W, H, n, dist.ctypes.data, maps=mb)
        texts[n] = log.text
    lines = [ln for ln in texts[5].splitlines()]
    launches = [(i, ln.split()[1], ln.split()[-1]) for i, ln in enumerate(lines) if ln.startswith("launch")]
    names = [k for _, k, _ in launches]
    assert [k for _, k, _ in [(0, ln.split()[1], 0) for ln in texts[2].splitlines() if ln.startswith("launch")]] == names, "a launch per image"
    assert len({s for _, _, s in launches}) == 1, texts[5]
    lib_stream = launches[0][2]
    ingest = [i for i, k, _ in launches if k.startswith("k_ingest_rgb")]
    emit = [i for i, k, _ in launches if k.startswith("k_emit_map")]
    assert len(ingest) == 2 and len(emit) == 1 and ingest[0] == launches[0][0], names
    assert sum(k.startswith("k_malta_rolled_batch") for k in names) == 1 and sum(k.startswith("k_combine") for k in names) == 1
    rec = [i for i, ln in enumerate(lines) if ln.startswith("record")]
    wait = [i for i, ln in enumerate(lines) if ln.startswith("wait")]
    assert len(rec) == len(wait) == 3, texts[5]           # the producer (one stream for both batches), the consumer twice
    assert rec[0] < wait[0] < ingest[0] and lines[wait[0]].split()[1] == lib_stream
    assert lines[rec[0]].split()[-1] != lib_stream
    assert ingest[1] < rec[1] < wait[1] < emit[0] and lines[wait[1]].split()[1] == lib_stream
    consumer = lines[rec[1]].split()[-1]
    assert emit[0] < rec[2] < wait[2] and lines[rec[2]].split()[-1] == lib_stream and lines[wait[2]].split()[1] == consumer
    syncs = [i for i, ln in enumerate(lines) if ln.startswith("stream_sync") and ln.split()[-1] == lib_stream]
    assert syncs and syncs[0] > wait[2], texts[5]         # the call waits for its own work, behind everything it enqueued


# ------------------------------------------------------------------ arguments ----
def test_argument_errors_come_before_any_device_call(L):
    lib = L.lib
    w, h, n = W, H, N
    refs, others = bbc.pairs(w, h, n)
    rsrc, osrc = bbc.lay_out(refs, "uint8", "NHWC"), bbc.lay_out(others, "uint8", "NHWC")
    good_r, good_o = rsrc.on(MEM)[0], osrc.on(MEM)[0]
    dist = np.full(n + 1, 7, np.float32)
    maps = np.full((n, h, w), 7, np.float32)

    def batch(**kw):
        a = dict(dict(ptr=osrc.buf.ctypes.data, dtype=capi.GZ_DT_U8, strides=osrc.strides), **kw)
        return device_batch(a["ptr"], a["dtype"], a["strides"])

    def mapb(**kw):
        a = dict(dict(ptr=maps.ctypes.data, dtype=capi.GZ_DT_F32, strides=(h * w, w, 1)), **kw)
        return device_map_batch(a["ptr"], a["dtype"], a["strides"])

    def call(r=good_r, o=good_o, d=dist.ctypes.data, m=None, ww=w, hh=h, nn=n, n_ref=n, cap=0):
        return lib.gz_butteraugli_batch(0, ww, hh, nn, None if r is None else C.byref(r), n_ref, None if o is None else C.byref(o), d, None,
                                        None if m is None else C.byref(m), cap)

    wrong_size, wrong_map = batch(), mapb()
    wrong_size.struct_size -= 8
    wrong_map.struct_size -= 8
    bad_batches = [batch(ptr=0), wrong_size, batch(dtype=-1), batch(dtype=capi.GZ_DT_U16), batch(dtype=5),
                   batch(strides=(-1, 3 * w, 3, 1)), batch(strides=(h * w * 3, -3 * w, 3, 1)), batch(strides=(h * w * 3, 3 * w, -3, 1)),
                   batch(strides=(h * w * 3, 3 * w, 3, -1)), batch(strides=(1 << 61, 3 * w, 3, 1)), batch(strides=(h * w * 3, 1 << 59, 3, 1))]
    bad_maps = [mapb(ptr=0), wrong_map, mapb(dtype=capi.GZ_DT_U8), mapb(dtype=capi.GZ_DT_U16), mapb(dtype=-1),
                mapb(strides=(-1, w, 1)), mapb(strides=(h * w, -w, 1)), mapb(strides=(h * w, w, -1)),
                mapb(strides=(0, w, 1)), mapb(strides=(h * w, 0, 1)), mapb(strides=(h * w, w, 0)),     # a stride of 0: elements on each other
                mapb(strides=(h * w - 1, w, 1)), mapb(strides=(h * w, w - 1, 1)), mapb(strides=(1, n, n * h - 1)),   # overlap by one element
                mapb(strides=(1 << 61, w, 1)), mapb(strides=(h * w, 1 << 59, 1))]
    launches, allocs = lib.gz_emu_launch_calls(), lib.gz_emu_alloc_calls()
    with enqueue_log(L) as log:
        for b in bad_batches:
            assert call(r=b) == -1 and call(o=b) == -1
        for m in bad_maps:
            assert call(m=m) == -1
        assert call(r=None) == -1 and call(o=None) == -1 and call(d=None) == -1
        assert call(d=dist.ctypes.data + 2) == -1                                   # distances: float32, so 4-byte aligned
        for nn, n_ref in ((0, 0), (-1, 1), (n, 0), (n, 2), (n, n + 1), (n, -1)):
            assert call(nn=nn, n_ref=n_ref) == -1, (nn, n_ref)
        for ww, hh in ((7, h), (w, 7), (0, h), (-1, h), (1 << 16, 8), (8, 1 << 16), (1500, 1000), (1250, 1200), (60000, 25)):
            assert call(ww=ww, hh=hh) == -1, (ww, hh)
    assert lib.gz_emu_launch_calls() == launches and lib.gz_emu_alloc_calls() == allocs
    assert log.text == "", log.text                                                # no copy, no event, no synchronise either
    assert (dist == 7).all() and (maps == 7).all()
    # what is allowed: stride_n = 0 for the inputs, one image with any stride_n, a map batch of one with stride_n = 0
    assert call(o=batch(strides=(0,) + tuple(osrc.strides[1:]))) == 0
    assert call(nn=1, n_ref=1, m=mapb(strides=(0, w, 1))) == 0
    assert call(m=mapb()) == 0 and call(r=good_r, n_ref=1) == 0
    exp = bbc.expected(oracle, refs, others)
    assert np.array_equal(dist[:n].view(np.uint32), bbc.expected(oracle, refs, others, broadcast=True)[0].view(np.uint32)) and dist[n] == 7
    assert call(m=mapb()) == 0
    bbc.assert_batch_equal((dist[:n].copy(), maps), exp, "after the refusals")


def test_the_product_library_checks_arguments_without_a_device():
    from guetzli_amd import build as gzbuild
    lib = Library(gzbuild.build()).lib
    a = np.zeros((2, 8, 8, 3), np.uint8)
    d = np.zeros(2, np.float32)
    good = device_batch(a.ctypes.data, capi.GZ_DT_U8, (192, 24, 3, 1))
    bad = device_batch(a.ctypes.data, capi.GZ_DT_U8, (192, -24, 3, 1))
    assert lib.gz_butteraugli_batch(0, 8, 8, 2, C.byref(good), 2, C.byref(bad), d.ctypes.data, None, None, 0) == -1
    assert lib.gz_butteraugli_batch(0, 8, 8, 2, C.byref(good), 3, C.byref(good), d.ctypes.data, None, None, 0) == -1
    assert lib.gz_butteraugli_batch(0, 1500, 1000, 2, C.byref(good), 2, C.byref(good), d.ctypes.data, None, None, 0) == -1
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:   # valid arguments: the device is asked for, and there is none -- no fallback
        assert lib.gz_butteraugli_batch(0, 8, 8, 2, C.byref(good), 2, C.byref(good), d.ctypes.data, None, None, 0) == -2


# ------------------------------------------------------------------ launches and allocations that fail ----
def failing_calls():
    refs, others = bbc.pairs(W, H, N)
    rsrc, osrc, one = bbc.lay_out(refs, "uint8", "NHWC"), bbc.lay_out(others, "uint8", "NHWC"), bbc.lay_out(refs[:1], "uint8", "NHWC")
    dist = np.zeros(N, np.float32)
    dest = bbc.MapBatchDestination(N, W, H, "bfloat16", "crop")
    mb = dest.on(MEM, CONSUMER)[0]
    cap = 2 * bbc.arena_bytes(W, H) + 64
    calls = {"pairs": lambda L: L.butteraugli_batch(rsrc.on(MEM, PRODUCER)[0], osrc.on(MEM, PRODUCER)[0], W, H, N, dist.ctypes.data, maps=mb),
             "pairs, chunked, no maps": lambda L: L.butteraugli_batch(rsrc.on(MEM)[0], osrc.on(MEM)[0], W, H, N, dist.ctypes.data, scratch_bytes=cap),
             "one reference": lambda L: L.butteraugli_batch(one.on(MEM)[0], osrc.on(MEM)[0], W, H, N, dist.ctypes.data, n_ref=1, maps=mb)}
    exp = {"pairs": bbc.expected(oracle, refs, others), "one reference": bbc.expected(oracle, refs, others, broadcast=True)}
    exp["pairs, chunked, no maps"] = exp["pairs"]
    return calls, exp, dest


@pytest.mark.parametrize("which", ["pairs", "pairs, chunked, no maps", "one reference"])
def test_every_launch_failing_in_turn(L, which):
    """The call fails with GZ_E_HIP, nothing stays allocated, the canvas around the maps keeps its sentinel, and the next
    call gives the checker's bits."""
    lib = L.lib
    calls, exp, dest = failing_calls()
    call, (ed, em) = calls[which], exp[which]
    base = live(lib)
    before = lib.gz_emu_launch_calls()
    assert np.array_equal(call(L).view(np.uint32), ed.view(np.uint32))
    n_launches = lib.gz_emu_launch_calls() - before
    assert n_launches >= 20 and live(lib) == base
    for k in range(n_launches):
        lib.gz_emu_fail_launch(k)
        try:
            with pytest.raises(capi.GuetzliAmdError, match="GZ_E_HIP"):
                call(L)
        finally:
            lib.gz_emu_fail_launch(-1)
        assert live(lib) == base, f"launch {k} failing leaves {live(lib)} behind"
        outside = dest.before.copy()
        dest.view_of(outside)[...] = dest.view_of(dest.raw)
        assert np.array_equal(dest.raw, outside), f"launch {k} failing: something between the maps' elements was written"
    assert np.array_equal(call(L).view(np.uint32), ed.view(np.uint32))
    if "no maps" not in which:
        dest.check(em, dest.raw, which)


def test_every_allocation_failing_in_turn(L):
    """GZ_E_NOMEM (or GZ_E_HIP), nothing left allocated, a working next call."""
    lib = L.lib
    calls, exp, dest = failing_calls()
    base = live(lib)
    for which, call in calls.items():
        before = lib.gz_emu_alloc_calls()
        call(L)
        n_allocs = lib.gz_emu_alloc_calls() - before
        assert n_allocs >= 5 and live(lib) == base
        for k in range(n_allocs):
            lib.gz_emu_fail_alloc(k)
            try:
                with pytest.raises(capi.GuetzliAmdError, match="GZ_E_NOMEM|GZ_E_HIP"):
                    call(L)
            finally:
                lib.gz_emu_fail_alloc(-1)
            assert live(lib) == base, f"{which}: allocation {k} failing leaves {live(lib)} behind"
        assert np.array_equal(call(L).view(np.uint32), exp[which][0].view(np.uint32)), which


# ------------------------------------------------------------------ the Python surface ----
import fake_device  # noqa: E402


def FakeDeviceArray(array, readonly=False):
    """fake_device's, under the array's own strides: these tests hand over slices and crops."""
    return fake_device.FakeDeviceArray(array, readonly, strides=array.strides)


@pytest.fixture()
def emulated(monkeypatch, L):
    """guetzli_amd.butteraugli_batch on the emulated library, with numpy memory for the tensors it allocates."""
    from guetzli_amd import encoder
    monkeypatch.setattr(encoder, "_pair_library", lambda: L)
    fake_device.install(monkeypatch)


def test_butteraugli_batch(emulated):
    import guetzli_amd
    w, h, n = W, H, 5
    refs, others = bbc.pairs(w, h, n)
    ed, em = bbc.expected(oracle, refs, others)
    d = guetzli_amd.butteraugli_batch(FakeDeviceArray(np.array(refs)), FakeDeviceArray(np.array(others)))
    assert d.array.shape == (n,) and np.array_equal(d.array.view(np.uint32), ed.view(np.uint32))
    d, m = guetzli_amd.butteraugli_batch(FakeDeviceArray(np.array(refs)), FakeDeviceArray(np.array(others)), distmap=True)
    bbc.assert_batch_equal((d.array, m.array), (ed, em), "NHWC, distmap=True")
    # NCHW float32 against a slice x[::2] of float16 NHWC; the maps into a float16 view inside a canvas
    chw = np.ascontiguousarray(bbc.dic.from_bytes(np.array(refs), "float32").transpose(0, 3, 1, 2))
    wide = np.zeros((2 * n, h, w, 3), np.float16)
    wide[::2] = bbc.dic.from_bytes(np.array(others), "float16").view(np.float16)
    canvas = np.full((n, h + 4, w + 9), 7, np.float16)
    view = canvas[:, 2:2 + h, 5:5 + w]
    d, m = guetzli_amd.butteraugli_batch(FakeDeviceArray(chw), FakeDeviceArray(wide[::2]), distmap=FakeDeviceArray(view))
    assert np.array_equal(d.array.view(np.uint32), ed.view(np.uint32))
    assert np.array_equal(view.view(np.uint16), bpc.emitted_map(em, "float16"))
    canvas[:, 2:2 + h, 5:5 + w] = 7
    assert (canvas == 7).all()
    # one reference for all, under a cap of two images
    bd, bm = bbc.expected(oracle, refs, others, broadcast=True)
    d, m = guetzli_amd.butteraugli_batch(FakeDeviceArray(np.array(refs[0])), FakeDeviceArray(np.array(others)), distmap=True,
                                         scratch_bytes=2 * bbc.arena_bytes(w, h) + 64)
    bbc.assert_batch_equal((d.array, m.array), (bd, bm), "one reference for all")


def test_butteraugli_batch_refuses(emulated, L):
    import guetzli_amd
    w, h, n = 33, 17, 2
    refs, others = (np.array(a) for a in bbc.pairs(w, h, n))
    F = FakeDeviceArray
    launches, allocs = L.lib.gz_emu_launch_calls(), L.lib.gz_emu_alloc_calls()
    with pytest.raises(ValueError, match="differ in size"):
        guetzli_amd.butteraugli_batch(F(refs), F(np.ascontiguousarray(others[:, :, :-1])))
    with pytest.raises(ValueError, match="as many, or one for all"):
        guetzli_amd.butteraugli_batch(F(np.concatenate([refs, refs[:1]])), F(others))
    with pytest.raises(ValueError, match="8 x 8"):
        guetzli_amd.butteraugli_batch(F(np.ascontiguousarray(refs[:, :7])), F(np.ascontiguousarray(others[:, :7])))
    with pytest.raises(ValueError, match="no alpha"):
        guetzli_amd.butteraugli_batch(F(refs), F(np.zeros((n, h, w, 4), np.uint8)))
    with pytest.raises(ValueError, match="no alpha"):
        guetzli_amd.butteraugli_batch(F(refs), F(np.zeros((n, 2, h, w), np.uint8)))
    with pytest.raises(ValueError, match="16-bit integer"):
        guetzli_amd.butteraugli_batch(F(refs), F(np.zeros((n, h, w, 3), np.uint16)))
    with pytest.raises(ValueError, match="1500000 pixels.*Comparator"):
        guetzli_amd.butteraugli_batch(F(np.zeros((1, 1000, 1500, 3), np.uint8)), F(np.zeros((1, 1000, 1500, 3), np.uint8)))
    with pytest.raises(ValueError, match=r"\[N,3,H,W\]"):
        guetzli_amd.butteraugli_batch(F(refs), F(others[0]))
    a = np.zeros((n, h, w), np.float32)
    with pytest.raises(ValueError, match="share an address"):
        guetzli_amd.butteraugli_batch(F(refs), F(others), distmap=F(np.broadcast_to(a[:1], (n, h, w))))
    with pytest.raises(ValueError, match="negative strides"):
        guetzli_amd.butteraugli_batch(F(refs), F(others), distmap=F(a[:, ::-1]))
    with pytest.raises(ValueError, match="shape"):
        guetzli_amd.butteraugli_batch(F(refs), F(others), distmap=F(np.zeros((n, w, h), np.float32)))
    with pytest.raises(ValueError, match="read-only"):
        guetzli_amd.butteraugli_batch(F(refs), F(others), distmap=F(a, readonly=True))
    with pytest.raises(TypeError):
        guetzli_amd.butteraugli_batch(F(refs), F(others), distmap=F(np.zeros((n, h, w), np.uint8)))
    with pytest.raises(TypeError):
        guetzli_amd.butteraugli_batch(F(refs), F(others), distmap=a)                    # host memory is no destination
    assert (L.lib.gz_emu_launch_calls(), L.lib.gz_emu_alloc_calls()) == (launches, allocs)
    assert not a.any()


# ------------------------------------------------------------------ bounds, under the host sanitizers ----
def test_the_batched_kernels_stay_inside_their_buffers(tmp_path):
    """tests/cpp/batch_bounds.cc: the batched ingest, one batched k_blur2d, a batched row / column pair, k_combine and the
    batched emit through the emulation's launch, with source, arenas and destination malloc'ed to exactly their last
    element, N = 3 at 9x17 and 67x33, built as a plain program with AddressSanitizer and UBSan.  Its own process, nothing
    preloaded."""
    exe = str(tmp_path / "batch_bounds")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-DGZ_EMU", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-w", "-I" + os.path.join(ROOT, "tests", "emu"), "-x", "c++",
                    os.path.join(ROOT, "tests", "cpp", "batch_bounds.cc"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all elements as expected, no access outside the buffers" in out.stdout
