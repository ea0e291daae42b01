"""Device-resident input on the MI355X: torch tensors on the GPU through gz_pack_rgb_device, gz_create_from_device and
guetzli_amd.process / process_many.  Here the 16-byte loads, the 16-bit widening and rintf are the device's own; the
same cases run through the CPU emulation in tests/test_device_input_emu.py."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import device_input_cases as dic
import images

pytestmark = pytest.mark.gpu

TARGET = 0.971769
Q5 = np.full((3, 64), 5, np.int32)
# the reference's output for tests/golden/bees.png at quality 95 (tests/test_gpu_parity.py: GOLDEN_JPEG_SHA[(444, 258, 95)])
BEES_Q95_SHA = "f2673f12a4856e020627fa151493a80b1cb2ee4dc81e28afc62dc089baf50242"


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def L():
    import guetzli_amd
    return guetzli_amd.load()


def on_device(torch, src):
    """(tensor that owns the memory, gz_device_image) of a dic.Source uploaded as it is, bit for bit."""
    from guetzli_amd.capi import device_image
    from guetzli_amd.encoder import DTYPE_CODES
    raw = src.storage.view(np.int16) if src.storage.dtype == np.uint16 else src.storage
    t = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
    assert t.data_ptr() % 64 == 0
    return t, device_image(t.data_ptr() + src.offset * src.itemsize, DTYPE_CODES[src.dtype], src.strides)


def as_tensor(torch, storage, dtype):
    """A torch tensor of `dtype` on the GPU with the elements of `storage` (dic.STORAGE), bit for bit."""
    if dtype in ("uint8", "float32"):
        return torch.from_numpy(np.ascontiguousarray(storage)).cuda()
    t = torch.from_numpy(np.ascontiguousarray(storage).view(np.int16)).cuda()
    return t.view(torch.float16 if dtype == "float16" else torch.bfloat16)


def sha(b):
    return hashlib.sha256(b).hexdigest()


# ------------------------------------------------------------------ pack parity ----
@pytest.mark.parametrize("layout", dic.LAYOUTS)
@pytest.mark.parametrize("dtype", dic.DTYPES)
def test_pack_parity(torch, L, dtype, layout):
    for src in dic.parity_sources(dtype, layout):
        keep, image = on_device(torch, src)
        got = L.pack_rgb_device(image, src.w, src.h)
        exp = dic.expected_bytes(src.logical, dtype)
        assert np.array_equal(got, exp), (dtype, layout, src.w, src.h, np.argwhere(got != exp)[:4])


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_pack_parity_exhaustive_floats(torch, L, dtype):
    """Every float16 / bfloat16 bit pattern, the float32 specials and ties, through the 16-byte paths and the
    element-wise one."""
    for src in dic.exhaustive_sources(dtype):
        keep, image = on_device(torch, src)
        got = L.pack_rgb_device(image, src.w, src.h)
        exp = dic.expected_bytes(src.logical, dtype)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, (dtype, src.strides, bad[:4], got[tuple(bad[0])], exp[tuple(bad[0])])


# ------------------------------------------------------------------ context parity ----
def evaluate(ctx):
    co = ctx.encode_rgb()
    cq = ctx.quantize(Q5)
    dist, dm, bm = ctx.compare()
    return co, cq, np.float32(dist), dm, bm


def test_context_from_device_equals_context_from_host(torch, L):
    w, h = 61, 43
    rgb = images.crop(w, h, 50, 40)
    with L.context(rgb, TARGET) as ctx:
        exp = evaluate(ctx)
    for dtype, layout in (("uint8", "HWC"), ("float32", "CHW")):
        keep, image = on_device(torch, dic.lay_out(dic.from_bytes(rgb, dtype), dtype, layout))
        with L.context_from_device(image, w, h, TARGET) as ctx:
            got = evaluate(ctx)
        for x, y, what in zip(got, exp, ("gz_encode_rgb coefficients", "quantised coefficients", "distance", "distance map", "block maxima")):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), (dtype, what)


# ------------------------------------------------------------------ whole encodes ----
@pytest.fixture(scope="module")
def bees():
    return images.bees()   # 444 x 258: rows of 1332 bytes, no multiple of 16


def test_bees_from_host_pixels(bees):
    import guetzli_amd
    assert sha(guetzli_amd.process(bees)[0]) == BEES_Q95_SHA


def test_bees_uint8_hwc_tensor(torch, bees):
    import guetzli_amd
    t = torch.from_numpy(bees).cuda()
    assert t.shape == (258, 444, 3) and t.dtype == torch.uint8
    assert sha(guetzli_amd.process(t)[0]) == BEES_Q95_SHA


def test_bees_float32_chw_tensor(torch, bees):
    import guetzli_amd
    t = as_tensor(torch, np.ascontiguousarray(dic.from_bytes(bees, "float32").transpose(2, 0, 1)), "float32")
    assert t.shape == (3, 258, 444) and t.dtype == torch.float32
    assert sha(guetzli_amd.process(t)[0]) == BEES_Q95_SHA


def test_bees_float16_chw_crop_of_a_padded_canvas(torch, bees):
    import guetzli_amd
    t = as_tensor(torch, np.ascontiguousarray(dic.from_bytes(bees, "float16").transpose(2, 0, 1)), "float16")
    canvas = torch.full((3, 258 + 10, 444 + 20), float("nan"), dtype=torch.float16, device="cuda")
    canvas[:, 5:5 + 258, 8:8 + 444] = t
    view = canvas[:, 5:5 + 258, 8:8 + 444]
    assert not view.is_contiguous() and view.stride() == (268 * 464, 464, 1)
    assert sha(guetzli_amd.process(view)[0]) == BEES_Q95_SHA


def test_the_producer_stream_is_waited_for(torch, bees):
    """The tensor is filled on a non-default stream -- behind work that keeps that stream busy -- and handed over at
    once, with no synchronise: the encoder queues behind torch's current stream.  (The enqueue-order test pins the
    record / wait pair; this exercises it on the device.)"""
    import guetzli_amd
    src = torch.from_numpy(bees).pin_memory()
    busy = torch.ones((2048, 2048), device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.zeros((258, 444, 3), dtype=torch.uint8, device="cuda")
        for _ in range(8):
            busy = busy @ busy * 0.0 + 1.0
        t.copy_(src, non_blocking=True)
        jpg, _ = guetzli_amd.process(t)
    torch.cuda.synchronize()
    assert sha(jpg) == BEES_Q95_SHA


# ------------------------------------------------------------------ small and batched ----
def test_an_image_too_small_for_a_context(torch):
    import guetzli_amd
    rgb = images.crop(16, 16, 100, 60)
    exp, _ = guetzli_amd.process(rgb)
    assert guetzli_amd.process(torch.from_numpy(rgb).cuda())[0] == exp
    chw = as_tensor(torch, np.ascontiguousarray(dic.from_bytes(rgb, "bfloat16").transpose(2, 0, 1)), "bfloat16")
    assert guetzli_amd.process(chw)[0] == exp


def test_process_many_equals_single_calls(torch):
    import guetzli_amd
    batch = np.stack([np.ascontiguousarray(images.crop(64, 64, 40 * k, 30 * k).transpose(2, 0, 1)) for k in range(4)])
    t = torch.from_numpy(batch).cuda()
    assert t.shape == (4, 3, 64, 64)
    many = guetzli_amd.process_many(t, workers=4)
    single = [guetzli_amd.process(t[k]) for k in range(4)]
    assert [m[0] for m in many] == [s[0] for s in single]
    assert [m[0] for m in many] == [guetzli_amd.process(np.ascontiguousarray(batch[k].transpose(1, 2, 0)))[0] for k in range(4)]
    assert len({m[0] for m in many}) == 4


def test_process_many_waits_for_the_callers_stream(torch, monkeypatch):
    """A batch filled on a non-default stream, behind work that keeps it busy, and handed to process_many at once: the
    encodes run on worker threads, whose own current stream is the default one, yet every image must be handed over with
    the CALLER's stream -- and give the bytes of the pixels that stream writes."""
    import guetzli_amd
    host = guetzli_amd.load_host()
    rgbs = [images.crop(64, 48, 40 * k, 30 * k) for k in range(4)]
    exp = [guetzli_amd.process(r)[0] for r in rgbs]
    src = torch.from_numpy(np.stack(rgbs)).pin_memory()
    handed, real = [], host.process_device

    def spy(*a, **kw):
        handed.append(kw["stream"])
        return real(*a, **kw)
    monkeypatch.setattr(host, "process_device", spy)
    busy = torch.ones((2048, 2048), device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.zeros((4, 48, 64, 3), dtype=torch.uint8, device="cuda")
        for _ in range(8):
            busy = busy @ busy * 0.0 + 1.0
        t.copy_(src, non_blocking=True)
        many = guetzli_amd.process_many(t, workers=4)
    torch.cuda.synchronize()
    assert s.cuda_stream != 0 and handed == [s.cuda_stream] * 4
    assert [m[0] for m in many] == exp


# ------------------------------------------------------------------ error codes ----
def test_a_tensor_on_another_device_is_refused(torch):
    import guetzli_amd
    t = torch.zeros((40, 40, 3), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(ValueError, match="device"):
        guetzli_amd.process(t, device=1)


def test_a_host_pointer_is_an_argument_error_not_a_fault(torch, L):
    """Ordinary (mapped, live) host memory where device memory is expected: GZ_E_ARG from every entry, and the process
    goes on working."""
    from guetzli_amd.capi import GZ_DT_U8, GuetzliAmdError, device_image
    w, h = 64, 48
    rgb = images.crop(w, h)
    image = device_image(rgb.ctypes.data, GZ_DT_U8, (3 * w, 3, 1))
    err = C.c_int(0)
    assert not L.lib.gz_create_from_device(0, w, h, C.byref(image), TARGET, C.byref(err))
    assert err.value == -1
    out = np.zeros_like(rgb)
    assert L.lib.gz_pack_rgb_device(0, C.byref(image), w, h, out.ctypes.data) == -1
    with L.context(rgb, TARGET) as ctx:
        with pytest.raises(GuetzliAmdError, match="GZ_E_ARG.*host pointer"):
            ctx.set_rgb_device(image)
        co = ctx.encode_rgb()          # the context is as it was
    keep, good = on_device(torch, dic.lay_out(rgb, "uint8", "HWC"))
    with L.context_from_device(good, w, h, TARGET) as ctx:
        assert np.array_equal(ctx.encode_rgb(), co)
