"""Device-resident pixels with alpha and 16-bit samples on the MI355X: torch tensors on the GPU through
gz_pack_rgb_device_pixels, gz_create_from_device_pixels and guetzli_amd.process / process_many with background=.  Here
the 16-byte loads, the integer division and the 16-bit widening are the device's own; the same cases run through the CPU
emulation in tests/test_device_alpha_emu.py.  The three PNG fixtures' raw samples, as tensors, must give the JPEGs the
unmodified reference wrote for the files."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import device_alpha_cases as dac
import device_input_cases as dic
import images

pytestmark = pytest.mark.gpu

TARGET = 0.971769
Q5 = np.full((3, 64), 5, np.int32)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def L():
    import guetzli_amd
    return guetzli_amd.load()


def upload(torch, storage):
    """The buffer on the GPU as it is, bit for bit (uint16 storage travels as int16)."""
    raw = storage.view(np.int16) if storage.dtype == np.uint16 else storage
    t = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
    assert t.data_ptr() % 64 == 0
    return t


def on_device(torch, src, bg=(0, 0, 0)):
    """(tensors that own the memory, gz_device_pixels) of a dac.Source -- or, opaque, of a dic.Source."""
    from guetzli_amd.capi import device_pixels
    from guetzli_amd.encoder import DTYPE_CODES
    t = upload(torch, src.storage)
    keep, alpha = [t], 0
    if getattr(src, "alpha_storage", None) is not None:
        ta = t if src.alpha_storage is src.storage else upload(torch, src.alpha_storage)
        keep.append(ta)
        alpha = ta.data_ptr() + src.alpha_offset * src.itemsize
    return keep, device_pixels(t.data_ptr() + src.offset * src.itemsize, DTYPE_CODES[src.dtype], src.strides, 0, alpha, bg)


def as_tensor(torch, storage, dtype):
    """A torch tensor of `dtype` on the GPU with the elements of `storage` (dac.STORAGE), bit for bit."""
    if dtype in ("uint8", "float32"):
        return torch.from_numpy(np.ascontiguousarray(storage)).cuda()
    t = torch.from_numpy(np.ascontiguousarray(storage).view(np.int16)).cuda()
    return t.view({"uint16": torch.uint16, "float16": torch.float16, "bfloat16": torch.bfloat16}[dtype])


def sha(b):
    return hashlib.sha256(b).hexdigest()


# ------------------------------------------------------------------ pack parity ----
@pytest.mark.parametrize("layout", dac.LAYOUTS)
@pytest.mark.parametrize("dtype", dac.DTYPES)
def test_pack_parity(torch, L, dtype, layout):
    for src, bg in dac.parity_sources(dtype, layout):
        keep, image = on_device(torch, src, bg)
        got = L.pack_rgb_device(image, src.w, src.h)
        exp = src.expected(bg)
        assert np.array_equal(got, exp), (dtype, layout, src.w, src.h, bg, np.argwhere(got != exp)[:4])


@pytest.mark.parametrize("layout", dic.LAYOUTS)
def test_pack_parity_opaque_uint16(torch, L, layout):
    rng = np.random.default_rng(5)
    for h in dac.HEIGHTS:
        for w in dac.WIDTHS:
            src = dac.lay_out_opaque(dac.random_storage("uint16", h * w * 3, rng).reshape(h, w, 3), "uint16", layout)
            keep, image = on_device(torch, src, (9, 99, 199))
            got = L.pack_rgb_device(image, w, h)
            assert np.array_equal(got, dac.expected_rgb(src.logical, None, "uint16")), (layout, w, h)


@pytest.mark.parametrize("layout", ["HWC_rgba", "HWC_rgba_base1"])
def test_every_value_alpha_pair_under_every_background(torch, L, layout):
    """All 65536 (v, a) pairs in every channel through the device's integer division: the four-vector path and element
    by element."""
    colour, alpha = dac.every_v_a_pair()
    src = dac.lay_out(colour, alpha, "uint8", layout)
    for bg in dac.EXHAUSTIVE_BACKGROUNDS:
        keep, image = on_device(torch, src, bg)
        got = L.pack_rgb_device(image, src.w, src.h)
        exp = src.expected(bg)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, (layout, bg, [(tuple(i), int(got[tuple(i)]), int(exp[tuple(i)])) for i in bad[:4]])


@pytest.mark.parametrize("layout", ["HWC_rgba", "CHW_rgba", "HWC_rgba_base1"])
def test_every_uint16_pattern_as_value_and_as_alpha(torch, L, layout):
    colour, alpha = dac.every_u16_pattern()
    src = dac.lay_out(colour, alpha, "uint16", layout)
    for bg in ((0, 0, 0), (255, 1, 128)):
        keep, image = on_device(torch, src, bg)
        assert np.array_equal(L.pack_rgb_device(image, src.w, src.h), src.expected(bg)), (layout, bg)


# ------------------------------------------------------------------ context parity ----
def rgba_case(w, h, x0, y0, seed):
    """(rgb bytes, alpha bytes, background, the host-blended bytes)."""
    rng = np.random.default_rng(seed)
    rgb = images.crop(w, h, x0, y0)
    alpha = rng.integers(0, 256, (h, w), dtype=np.uint8)
    alpha[::3, ::2] = 255
    alpha[1::4, 1::5] = 0
    bg = (30, 144, 255)
    return rgb, alpha, bg, dac.blend(rgb, alpha[..., None], bg)


def evaluate(ctx):
    co = ctx.encode_rgb()
    cq = ctx.quantize(Q5)
    dist, dm, bm = ctx.compare()
    return co, cq, np.float32(dist), dm, bm


def test_context_from_rgba_pixels_equals_context_from_the_blended_bytes(torch, L):
    w, h = 61, 43
    rgb, alpha, bg, blended = rgba_case(w, h, 50, 40, 1)
    with L.context(blended, TARGET) as ctx:
        exp = evaluate(ctx)
    for src in (dac.lay_out(rgb, alpha, "uint8", "HWC_rgba"),
                dac.lay_out(dic.from_bytes(rgb, "float32"), dic.from_bytes(alpha, "float32"), "float32", "CHW_rgba")):
        keep, image = on_device(torch, src, bg)
        with L.context_from_device(image, w, h, TARGET) as ctx:
            got = evaluate(ctx)
        for x, y, what in zip(got, exp, ("gz_encode_rgb coefficients", "quantised coefficients", "distance", "distance map", "block maxima")):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), (src.dtype, what)


# ------------------------------------------------------------------ the reference's JPEGs of the PNG fixtures ----
@pytest.fixture(scope="module")
def samples():
    return dac.fixture_samples()   # (asserts that the rule turns them into each fixture's rgb_sha256)


@pytest.mark.parametrize("name,shape,dtype", [("png_rgba8_160x120_q95", (120, 160, 4), "uint8"),
                                              ("png_rgb16_160x120_q95", (120, 160, 3), "uint16"),
                                              ("png_greyalpha16_interlaced_160x120_q90", (120, 160, 2), "uint16")])
def test_a_fixtures_samples_as_a_tensor_give_the_reference_jpeg(torch, samples, name, shape, dtype):
    import guetzli_amd
    s, dt = samples[name]
    gold = dac.fixture(name)
    t = as_tensor(torch, s, dt)
    assert tuple(t.shape) == shape and dt == dtype and str(t.dtype) == "torch." + dtype
    jpg, _ = guetzli_amd.process(t, quality=gold["quality"], background=0)
    assert (len(jpg), sha(jpg)) == (gold["bytes"], gold["jpeg_sha256"])


def test_the_rgba_fixture_as_float32_planes(torch, samples):
    import guetzli_amd
    s, _ = samples["png_rgba8_160x120_q95"]
    gold = dac.fixture("png_rgba8_160x120_q95")
    t = as_tensor(torch, np.ascontiguousarray(dic.from_bytes(s, "float32").transpose(2, 0, 1)), "float32")
    assert tuple(t.shape) == (4, 120, 160) and t.dtype == torch.float32
    jpg, _ = guetzli_amd.process(t, quality=gold["quality"], background=0)
    assert (len(jpg), sha(jpg)) == (gold["bytes"], gold["jpeg_sha256"])


# ------------------------------------------------------------------ small and batched ----
def test_an_rgba_image_too_small_for_a_context(torch):
    import guetzli_amd
    rgb, alpha, bg, blended = rgba_case(16, 16, 100, 60, 3)
    exp, _ = guetzli_amd.process(blended)
    t = torch.from_numpy(np.concatenate([rgb, alpha[..., None]], -1)).cuda()
    assert tuple(t.shape) == (16, 16, 4)
    assert guetzli_amd.process(t, background=bg)[0] == exp
    assert guetzli_amd.process(t.permute(2, 0, 1).contiguous(), background=bg)[0] == exp


def test_process_many_of_an_rgba_batch_equals_single_calls(torch):
    import guetzli_amd
    cases = [rgba_case(64, 64, 40 * k, 30 * k, 10 + k) for k in range(4)]
    bg = cases[0][2]
    t = torch.from_numpy(np.stack([np.concatenate([c[0], c[1][..., None]], -1) for c in cases])).cuda()
    assert tuple(t.shape) == (4, 64, 64, 4)
    many = guetzli_amd.process_many(t, workers=4, background=bg)
    single = [guetzli_amd.process(t[k], background=bg) for k in range(4)]
    assert [m[0] for m in many] == [s[0] for s in single]
    assert [m[0] for m in many] == [guetzli_amd.process(c[3])[0] for c in cases]
    assert len({m[0] for m in many}) == 4


# ------------------------------------------------------------------ error codes ----
def test_an_alpha_pointer_in_host_memory_is_an_argument_error_not_a_fault(torch, L):
    """Colours on the GPU, the alpha pointer ordinary (mapped, live) host memory: GZ_E_ARG from every entry, the message
    names alpha, and the process goes on working."""
    from guetzli_amd.capi import GZ_DT_U8, GuetzliAmdError, device_pixels
    w, h = 64, 48
    rgb, alpha, bg, blended = rgba_case(w, h, 0, 0, 5)
    t = torch.from_numpy(rgb).cuda()
    mask = np.ascontiguousarray(np.repeat(alpha[..., None], 3, -1))   # (alpha moves with the colours' strides)
    image = device_pixels(t.data_ptr(), GZ_DT_U8, (3 * w, 3, 1), 0, mask.ctypes.data, bg)
    err = C.c_int(0)
    assert not L.lib.gz_create_from_device_pixels(0, w, h, C.byref(image), TARGET, C.byref(err))
    assert err.value == -1
    out = np.zeros_like(rgb)
    assert L.lib.gz_pack_rgb_device_pixels(0, C.byref(image), w, h, out.ctypes.data) == -1
    with L.context(blended, TARGET) as ctx:
        with pytest.raises(GuetzliAmdError, match="GZ_E_ARG.*alpha.*host pointer"):
            ctx.set_rgb_device(image)
        co = ctx.encode_rgb()          # the context is as it was
    tm = torch.from_numpy(mask).cuda()   # the same mask on the GPU, in an allocation of its own
    good = device_pixels(t.data_ptr(), GZ_DT_U8, (3 * w, 3, 1), 0, tm.data_ptr(), bg)
    assert np.array_equal(L.pack_rgb_device(good, w, h), blended)
    with L.context_from_device(good, w, h, TARGET) as ctx:
        assert np.array_equal(ctx.encode_rgb(), co)
