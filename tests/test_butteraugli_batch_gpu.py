"""gz_butteraugli_batch on the MI355X: the cases of tests/butteraugli_batch_cases.py, which
tests/test_butteraugli_batch_emu.py runs through the CPU emulation, on memory of torch tensors -- here the grid's image
index, the 16-byte paths and the atomics on the per-image result words are the device's own -- and
guetzli_amd.butteraugli_batch on torch tensors.  Expectations come from the checkers under oracle/ (the CPU restatement,
and the unmodified reference behind oracle/_ref where it is built) and from this library's sequential path; every
comparison is bitwise."""
import ctypes as C

import numpy as np
import pytest

import butteraugli_batch_cases as bbc
import butteraugli_pair_cases as bpc
from checkers import bits, oracle, ref

pytestmark = pytest.mark.gpu

CHK = ref or oracle
W, H = 67, 33


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def L(torch):   # (behind torch: the process then has one HIP runtime, torch's, which the library's NEEDED entry resolves to)
    import guetzli_amd
    return guetzli_amd.load()


@pytest.fixture(scope="module")
def mem(torch):
    class TorchMemory:
        """Device memory: a numpy buffer copied to the GPU (torch's allocations are aligned as the cases assume)."""

        def put(self, array):
            t = torch.from_numpy(np.ascontiguousarray(array)).cuda()
            assert t.data_ptr() % 64 == 0
            return t

        def address(self, handle):
            return handle.data_ptr()

        def get(self, handle):
            return handle.cpu().numpy()
    return TorchMemory()


# ------------------------------------------------------------------ the cases shared with the emulation ----
@pytest.mark.parametrize("shape", bbc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_parity_at_every_shape(L, mem, shape):
    bbc.case_parity(L, mem, CHK, shape[0], shape[1], 3)


@pytest.mark.parametrize("n", bbc.BATCH_SIZES)
def test_parity_at_every_batch_size(L, mem, n):
    bbc.case_parity(L, mem, CHK, W, H, n)


@pytest.mark.parametrize("shape", bbc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_reference_for_all(L, mem, shape):
    bbc.case_broadcast(L, mem, CHK, shape[0], shape[1], 3)


@pytest.mark.parametrize("layout", bbc.IN_LAYOUTS)
@pytest.mark.parametrize("dtype", bbc.DTYPES)
def test_every_way_in(L, mem, dtype, layout):
    bbc.case_way_in(L, mem, CHK, dtype, layout)


@pytest.mark.parametrize("layout", bbc.MAP_LAYOUTS)
@pytest.mark.parametrize("dtype", bpc.MAP_DTYPES)
def test_maps_of_every_type_and_layout(L, mem, dtype, layout):
    bbc.case_maps(L, mem, CHK, dtype, layout)


def test_chunks_of_two_give_the_unchunked_bits(L, mem):
    whole = bbc.case_chunking(L, mem)
    refs, others = bbc.pairs(W, H, 5)
    bbc.assert_batch_equal(whole, bbc.expected(CHK, refs, others), "the unchunked batch")


# ------------------------------------------------------------------ arguments ----
def test_a_host_pointer_is_an_argument_error_not_a_fault(torch, L, mem):
    """Ordinary host memory where device memory is expected -- either batch, the distances, the maps: GZ_E_ARG (by the
    return code alone), nothing is written, and the next call works."""
    from guetzli_amd.capi import GZ_DT_F32, GZ_DT_U8, device_batch, device_map_batch
    n = 3
    refs, others = bbc.pairs(W, H, n)
    rsrc, osrc = bbc.lay_out(refs, "uint8", "NHWC"), bbc.lay_out(others, "uint8", "NHWC")
    (rb, r_held), (ob, o_held) = rsrc.on(mem), osrc.on(mem)
    dist = torch.zeros(n, dtype=torch.float32, device="cuda")
    maps = torch.zeros((n, H, W), dtype=torch.float32, device="cuda")
    good_maps = device_map_batch(maps.data_ptr(), GZ_DT_F32, (H * W, W, 1))
    host_batch = device_batch(osrc.buf.ctypes.data, GZ_DT_U8, osrc.strides)
    host_dist, host_maps = np.zeros(n, np.float32), np.zeros((n, H, W), np.float32)
    on_host = device_map_batch(host_maps.ctypes.data, GZ_DT_F32, (H * W, W, 1))

    def call(r=rb, o=ob, d=dist.data_ptr(), m=good_maps):
        return L.lib.gz_butteraugli_batch(0, W, H, n, C.byref(r), n, C.byref(o), d, None, C.byref(m), 0)

    assert call(r=host_batch) == -1 and call(o=host_batch) == -1
    assert call(d=host_dist.ctypes.data) == -1 and call(m=on_host) == -1
    torch.cuda.synchronize()
    assert not host_maps.any() and not host_dist.any() and not bool(dist.any()) and not bool(maps.any())
    assert call() == 0
    bbc.assert_batch_equal((dist.cpu().numpy(), maps.cpu().numpy()), bbc.expected(CHK, refs, others), "after the refusals")


# ------------------------------------------------------------------ guetzli_amd.butteraugli_batch on torch tensors ----
def tensor_of(torch, rgb, dtype):
    """A GPU tensor [n][h][w][3] of `dtype` whose bytes, by the ingest rule, are `rgb`."""
    t = torch.from_numpy(np.ascontiguousarray(bbc.dic.from_bytes(np.array(rgb), dtype))).cuda()
    return t.view(torch.int16).view(getattr(torch, dtype)) if dtype in ("float16", "bfloat16") else t


def test_butteraugli_batch_of_torch_tensors(torch):
    import guetzli_amd
    n = 5
    refs, others = bbc.pairs(W, H, n)
    ed, em = bbc.expected(CHK, refs, others)
    r8, o8 = tensor_of(torch, refs, "uint8"), tensor_of(torch, others, "uint8")
    d = guetzli_amd.butteraugli_batch(r8, o8)
    assert d.is_cuda and d.dtype == torch.float32 and tuple(d.shape) == (n,)
    assert np.array_equal(d.cpu().numpy().view(np.uint32), ed.view(np.uint32))
    d, m = guetzli_amd.butteraugli_batch(r8, o8, distmap=True)
    assert m.is_cuda and m.dtype == torch.float32 and tuple(m.shape) == (n, H, W)
    bbc.assert_batch_equal((d.cpu().numpy(), m.cpu().numpy()), (ed, em), "uint8 NHWC")
    # NCHW float32 against a slice x[::2] of bfloat16 NHWC, the maps into a float16 crop view of a sentinel canvas
    chw = tensor_of(torch, refs, "float32").permute(0, 3, 1, 2).contiguous()
    wide = torch.zeros((2 * n, H, W, 3), dtype=torch.bfloat16, device="cuda")
    wide[::2] = tensor_of(torch, others, "bfloat16")
    canvas = torch.full((n, H + 5, W + 19), -7.0, dtype=torch.float16, device="cuda")
    view = canvas[:, 3:3 + H, 8:8 + W]
    d, m = guetzli_amd.butteraugli_batch(chw, wide[::2], distmap=view)
    assert m is view and np.array_equal(d.cpu().numpy().view(np.uint32), ed.view(np.uint32))
    got = view.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, bpc.emitted_map(em, "float16"))
    canvas[:, 3:3 + H, 8:8 + W] = -7.0
    assert bool((canvas == -7.0).all())   # nothing around the crops was touched
    # one reference for all (a 3-D image), host arrays, a cap of two images
    bd, bm = bbc.expected(CHK, refs, others, broadcast=True)
    d, m = guetzli_amd.butteraugli_batch(r8[0], np.array(others), distmap=True, scratch_bytes=2 * bbc.arena_bytes(W, H) + 64)
    bbc.assert_batch_equal((d.cpu().numpy(), m.cpu().numpy()), (bd, bm), "one reference for all")
    # pair i is butteraugli(reference[i], distorted[i])
    for i in (1, 4):
        assert bits(np.float32(guetzli_amd.butteraugli(r8[i], o8[i]))) == bits(ed[i])


def test_the_current_stream_sees_distances_and_maps(torch):
    """The batches produced on a busy non-default stream just before the call, a consumer enqueued on it right after:
    it reads the distances and the maps, with no synchronisation in between."""
    import guetzli_amd
    n = 3
    refs, others = bbc.pairs(W, H, n)
    ed, em = bbc.expected(CHK, refs, others)
    staged_r, staged_o = torch.from_numpy(np.array(refs)).cuda(), torch.from_numpy(np.array(others)).cuda()
    busy = torch.ones((2048, 2048), device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(8):
            busy = busy @ busy * 0.0 + 1.0
        r, o = torch.zeros_like(staged_r), torch.zeros_like(staged_o)
        r.copy_(staged_r)
        o.copy_(staged_o)                                     # the producers, on s
        out = torch.zeros((n, H, W), dtype=torch.float32, device="cuda")
        d, m = guetzli_amd.butteraugli_batch(r, o, distmap=out)
        copy_d, copy_m = d.clone(), out.clone()               # the consumers, on s
    torch.cuda.synchronize()
    assert m is out
    bbc.assert_batch_equal((copy_d.cpu().numpy(), copy_m.cpu().numpy()), (ed, em), "what the consumer read")


def test_butteraugli_batch_refuses(torch):
    import guetzli_amd
    n, w, h = 2, 33, 17
    refs, others = (torch.from_numpy(np.array(a)).cuda() for a in bbc.pairs(w, h, n))
    with pytest.raises(ValueError, match="differ in size"):
        guetzli_amd.butteraugli_batch(refs, others[:, :, :-1])
    with pytest.raises(ValueError, match="as many, or one for all"):
        guetzli_amd.butteraugli_batch(torch.cat([refs, refs[:1]]), others)
    with pytest.raises(ValueError, match="8 x 8"):
        guetzli_amd.butteraugli_batch(refs[:, :7], others[:, :7])
    with pytest.raises(ValueError, match="no alpha"):
        guetzli_amd.butteraugli_batch(refs, torch.zeros((n, h, w, 4), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="16-bit integer"):
        guetzli_amd.butteraugli_batch(refs, torch.zeros((n, h, w, 3), dtype=torch.uint16, device="cuda"))
    big = torch.zeros((1, 1000, 1500, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="1500000 pixels.*Comparator"):
        guetzli_amd.butteraugli_batch(big, big)
    with pytest.raises(ValueError, match="device"):
        guetzli_amd.butteraugli_batch(refs, others, device=1)
    with pytest.raises(ValueError, match="share an address"):
        guetzli_amd.butteraugli_batch(refs, others, distmap=torch.zeros((1, h, w), device="cuda").expand(n, h, w))
    with pytest.raises(ValueError, match="shape"):
        guetzli_amd.butteraugli_batch(refs, others, distmap=torch.zeros((n, w, h), device="cuda"))
    with pytest.raises(TypeError):
        guetzli_amd.butteraugli_batch(refs, others, distmap=torch.zeros((n, h, w), dtype=torch.float64, device="cuda"))
    d = guetzli_amd.butteraugli_batch(refs, others)
    assert np.array_equal(d.cpu().numpy().view(np.uint32), bbc.expected(CHK, *bbc.pairs(w, h, n))[0].view(np.uint32))


# ------------------------------------------------------------------ the workload's shape, once ----
def test_64_crops_of_256x256_equal_the_sequential_path(torch, L, mem):
    """64 x 256x256 uint8 pairs -- the shape the batch is for: 64 distances and maps equal to one context per reference
    and one gz_compare_device_pixels per pair."""
    import guetzli_amd
    n, w, h = 64, 256, 256
    rng = np.random.default_rng(20261020)
    refs = np.stack([bbc.photo_crop(w, h, 16 * (i % 8), 12 * (i // 8)) for i in range(n)])
    others = refs.copy()
    for i in range(n):   # every pair distorted another way: noise of another strength and draw, or a shift
        if i % 2 == 0:
            others[i] = np.clip(refs[i].astype(np.int16) + rng.integers(-2 - i % 7, 3 + i % 7, refs[i].shape), 0, 255).astype(np.uint8)
        else:
            others[i] = np.roll(refs[i], 1 + i % 4, axis=(i // 2) % 2)
    exp = bbc.sequential(L, mem, refs, others)
    d, m = guetzli_amd.butteraugli_batch(torch.from_numpy(refs).cuda(), torch.from_numpy(others).cuda(), distmap=True)
    bbc.assert_batch_equal((d.cpu().numpy(), m.cpu().numpy()), exp, "64 x 256x256")
    assert len(set(exp[0].view(np.uint32).tolist())) > n // 2   # (different pairs: the 32 noise draws alone are independent)
