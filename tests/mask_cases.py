"""Shared by tests/test_mask_emu.py (CPU emulation: "device memory" is host memory) and tests/test_mask_gpu.py (memory of
the MI355X): butteraugli's masking on the device -- gz_opsin_device, gz_mask_device, gz_adaptive_quantization.

What judges the results: a checker's opsin(lin) and mask(xyb0, xyb1) -- the CPU restatement under oracle/, and the
unmodified reference where it is built -- of the float32 planes each image's elements become: fields.linear(bytes) for
8-bit samples, butteraugli_linear_cases.planes_of for linear ones.  Every comparison is bitwise.

A case takes `mem`, which says where device memory is (butteraugli_pair_cases.HostMemory here, the GPU suite's own for
torch tensors)."""
import numpy as np

import butteraugli_linear_cases as blc
import butteraugli_pair_cases as bpc
import device_input_cases as dic
import device_output_cases as doc
import fields
from checkers import assert_bits_equal
from guetzli_amd.capi import GZ_SAMPLES_LINEAR, GZ_SAMPLES_SRGB8, device_output

DTYPES = ("float32", "float16", "bfloat16")
QUANT_SIZES = ((16, 16), (17, 16), (33, 17), (64, 48), (70, 37))   # the minimum (both blurs are all border) .. over a 64-wide tile and two 16-row tiles
MASK_SIZES = ((8, 8), (9, 15), (33, 17), (64, 48))
# CHW contiguous, HWC, a CHW crop at an odd element offset (no plane base is 16-byte aligned), an HWC crop
OUT_LAYOUTS = ("CHW", "HWC", "CHW_crop_base1", "HWC_crop")
QUANT_LAYOUTS = ("contiguous", "crop", "base1", "transposed")
# w mod P in {0, 1, P - 1} for P = 4 (float32) and P = 8 (the 16-bit types)
OUT_WIDTHS = {"float32": (16, 17, 19), "float16": (16, 17, 23), "bfloat16": (16, 17, 23)}


# ------------------------------------------------------------------ images ----
def noise(w, h, seed=0):
    rng = np.random.default_rng(fields.SEED + w * 131 + h + seed)
    return (rng.random((3, h, w), dtype=np.float32) * np.float32(255)).astype(np.float32)


def ramp(w, h):
    """A ramp along both axes: R along x, B along y, G along the diagonal."""
    x = np.arange(w, dtype=np.float32)[None, :] / np.float32(w - 1)
    y = np.arange(h, dtype=np.float32)[:, None] / np.float32(h - 1)
    return np.stack([x * 255 + 0 * y, (x + y) * np.float32(127.5), y * 255 + 0 * x]).astype(np.float32)


def edges(w, h):
    """Half 0 / half 255, with one row at 128."""
    a = np.zeros((3, h, w), np.float32)
    a[:, :, w // 2:] = 255
    a[:, h // 2, :] = 128
    return a


CONTENTS = (("noise", noise), ("ramp", ramp), ("edges", edges))


def linear_source(planes, dtype="float32", layout="CHW", scale=1.0):
    return dic.lay_out(blc.image_of_planes(planes, dtype, scale), dtype, layout)


# ------------------------------------------------------------------ expectations, computed once ----
_quant, _mask, _opsin = {}, {}, {}


def _frozen(a):
    a.setflags(write=False)
    return a


def expected_opsin(chk, lin):
    key = (chk.name, lin.shape, lin.tobytes())
    if key not in _opsin:
        _opsin[key] = _frozen(chk.opsin(np.ascontiguousarray(lin, np.float32)))
    return _opsin[key]


def expected_mask(chk, lin0, lin1):
    """(mask, mask_dc) float32 [3][h][w] of Mask(opsin(lin0), opsin(lin1))."""
    key = (chk.name, lin0.shape, lin0.tobytes(), lin1.tobytes())
    if key not in _mask:
        m, dc = chk.mask(expected_opsin(chk, lin0), expected_opsin(chk, lin1))
        _mask[key] = (_frozen(m), _frozen(dc))
    return _mask[key]


def expected_quant(chk, lin):
    """ButteraugliAdaptiveQuantization: plane 1 of Mask applied to the linear planes themselves."""
    key = (chk.name, lin.shape, lin.tobytes())
    if key not in _quant:
        _quant[key] = _frozen(np.ascontiguousarray(chk.mask(np.ascontiguousarray(lin, np.float32), np.ascontiguousarray(lin, np.float32))[0][1]))
    return _quant[key]


# ------------------------------------------------------------------ destinations ----
def store_paths(address, itemsize, strides, planes=3):
    """emit_mask_wide_bits restated: per plane, whether a full group may leave as one 16-byte store."""
    sy, sx, sc = strides
    p = 16 // itemsize
    return {"wide" if sx == 1 and sy % p == 0 and (address + c * sc * itemsize) % 16 == 0 else "elementwise" for c in range(planes)}


class Out:
    """A device_output_cases destination for three float planes, in device memory."""

    def __init__(self, mem, w, h, dtype="float32", layout="CHW_crop_base1", stream=0):
        self.mem, self.dest = mem, doc.destination(w, h, dtype, layout)
        self.handle = mem.put(self.dest.raw)
        address = mem.address(self.handle) + self.dest.offset * self.dest.itemsize
        self.arg = device_output(address, bpc.MAP_CODES[dtype], self.dest.strides, stream)
        self.paths = store_paths(address, self.dest.itemsize, self.dest.strides)

    def raw(self):
        return np.ascontiguousarray(self.mem.get(self.handle)).view(np.uint8).ravel()

    def check(self, planes, what):
        """Every element is the element rule's of float32 [3][h][w] `planes`, every byte around them the sentinel."""
        d = self.dest
        exp = d.before.copy()
        want = bpc.emitted_map(np.ascontiguousarray(np.asarray(planes, np.float32).transpose(1, 2, 0)), d.dtype)
        d.image_of(exp)[...] = want
        raw = self.raw()
        got, img = d.image_of(raw), d.image_of(exp)
        gb = got.view(np.uint32 if d.itemsize == 4 else np.uint16)
        eb = img.view(np.uint32 if d.itemsize == 4 else np.uint16)
        assert (gb == eb).all(), (what, "image", d.dtype, d.strides, d.w, d.h, np.argwhere(gb != eb)[:4], gb[gb != eb][:4], eb[gb != eb][:4])
        bad = np.flatnonzero(raw != exp)
        assert bad.size == 0, (what, "outside the image", d.dtype, d.strides, d.w, d.h, bad[:8])

    def untouched(self, what):
        assert np.array_equal(self.raw(), self.dest.before), (what, "a destination that was not asked for was written")


class QuantOut:
    """A butteraugli_pair_cases map destination, in device memory."""

    def __init__(self, mem, w, h, dtype="float32", layout="crop", stream=0):
        self.mem, self.dest = mem, bpc.map_destination(w, h, dtype, layout)
        self.arg, self.handle = self.dest.on(mem, stream)
        address = mem.address(self.handle) + self.dest.offset * self.dest.itemsize
        self.paths = store_paths(address, self.dest.itemsize, self.dest.strides + (0,), planes=1)

    def check(self, plane, what):
        self.dest.check(plane, np.ascontiguousarray(self.mem.get(self.handle)).view(np.uint8).ravel(), what=what)


def quant_of(L, mem, src, scale=1.0, dtype="float32", layout="crop"):
    """gz_adaptive_quantization of a Source -> (QuantOut, clamped)."""
    px, held = blc.pixels_of(mem, src)
    out = QuantOut(mem, src.w, src.h, dtype, layout)
    clamped = L.adaptive_quantization(px, src.w, src.h, out.arg, scale)
    del held
    return out, clamped


def pixels(mem, src, samples):
    if samples == GZ_SAMPLES_LINEAR:
        return blc.pixels_of(mem, src)
    return bpc.pixels_of(mem, src)


# ------------------------------------------------------------------ 1. the quantisation field ----
def case_quant_parity(L, mem, chk):
    for w, h in QUANT_SIZES:
        for name, make in CONTENTS:
            lin = make(w, h)
            exp = expected_quant(chk, lin)
            assert exp.max() >= 1.05 * exp.min(), (name, w, h, exp.min(), exp.max())   # (a constant output cannot pass)
            out, clamped = quant_of(L, mem, linear_source(lin))
            out.check(exp, f"quantisation field of {name} {w}x{h}")
            assert clamped == 0


# ------------------------------------------------------------------ 2. Mask ----
def linear_pairs(w, h):
    """(name, planes0, planes1) of tests/fields.py pairs: linear [0, 255] fields off the sRGB table's values -- the
    originals and candidates butteraugli_linear_cases.parity_pairs takes, so that a case stays within seconds."""
    for name, _, lin0, lin1 in fields.pairs(w, h, only=("noise", "primaries")):
        if name.split("/")[1] in ("off_table", "jpeg_error_x3", "inverse"):
            yield name, lin0, lin1


def byte_pairs(w, h):
    for name in ("photo", "noise_flat"):
        yield (name,) + tuple(bpc.pair(name, w, h))


def check_mask(L, mem, chk, samples, src0, src1, lin0, lin1, what, request="both"):
    """One gz_mask_device call: the requested destinations hold the checker's planes, the other one its sentinel."""
    w, h = src0.w, src0.h
    em, edc = expected_mask(chk, lin0, lin0 if lin1 is None else lin1)
    p0, k0 = pixels(mem, src0, samples)
    p1, k1 = (None, None) if src1 is None else pixels(mem, src1, samples)
    m, dc = Out(mem, w, h, "float32", "CHW_crop_base1"), Out(mem, w, h, "float32", "HWC_crop")
    clamped = L.mask_device(p0, p1, w, h, m.arg if request != "dc" else None, dc.arg if request != "mask" else None, samples)
    assert clamped == 0
    if request != "dc":
        m.check(em, f"mask of {what} {w}x{h}")
    else:
        m.untouched(what)
    if request != "mask":
        dc.check(edc, f"mask_dc of {what} {w}x{h}")
    else:
        dc.untouched(what)


def case_mask_parity(L, mem, chk):
    for w, h in MASK_SIZES:
        for n, (name, lin0, lin1) in enumerate(linear_pairs(w, h)):
            s0, s1 = linear_source(lin0, layout="CHW"), linear_source(lin1, layout="HWC")
            check_mask(L, mem, chk, GZ_SAMPLES_LINEAR, s0, s1, lin0, lin1, name)
            check_mask(L, mem, chk, GZ_SAMPLES_LINEAR, s1, s0, lin1, lin0, name + " swapped")
            if n == 0:
                check_mask(L, mem, chk, GZ_SAMPLES_LINEAR, s1, None, lin1, None, name + " with itself")
                check_mask(L, mem, chk, GZ_SAMPLES_LINEAR, s0, s1, lin0, lin1, name, "mask")
                check_mask(L, mem, chk, GZ_SAMPLES_LINEAR, s0, s1, lin0, lin1, name, "dc")
        for n, (name, rgb0, rgb1) in enumerate(byte_pairs(w, h)):
            s0, s1 = dic.lay_out(rgb0, "uint8", "HWC"), dic.lay_out(rgb1, "uint8", "CHW")
            l0, l1 = fields.linear(rgb0), fields.linear(rgb1)
            check_mask(L, mem, chk, GZ_SAMPLES_SRGB8, s0, s1, l0, l1, name + " (8-bit)")
            check_mask(L, mem, chk, GZ_SAMPLES_SRGB8, s1, s0, l1, l0, name + " (8-bit) swapped")
            if n == 0:
                check_mask(L, mem, chk, GZ_SAMPLES_SRGB8, s0, None, l0, None, name + " (8-bit) with itself")
                check_mask(L, mem, chk, GZ_SAMPLES_SRGB8, s0, s1, l0, l1, name + " (8-bit)", "mask")
                check_mask(L, mem, chk, GZ_SAMPLES_SRGB8, s0, s1, l0, l1, name + " (8-bit)", "dc")
        if (w, h) == (33, 17):   # the two images' halves of DiffPrecompute differ, so the mask of a pair is not the mask of one image
            name, lin0, lin1 = next(iter(linear_pairs(w, h)))
            assert not np.array_equal(expected_mask(chk, lin0, lin1)[0], expected_mask(chk, lin0, lin0)[0])


# ------------------------------------------------------------------ 3. the opsin image ----
def case_opsin_parity(L, mem, chk):
    for w, h in MASK_SIZES:
        lin = noise(w, h)
        src = linear_source(lin, layout="HWC")
        px, held = blc.pixels_of(mem, src)
        out = Out(mem, w, h)
        assert L.opsin_device(px, w, h, out.arg, GZ_SAMPLES_LINEAR) == 0
        out.check(expected_opsin(chk, lin), f"opsin image of linear noise {w}x{h}")
        rgb = bpc.pair("photo", w, h)[0]
        px, held = bpc.pixels_of(mem, dic.lay_out(rgb, "uint8", "HWC"))
        out = Out(mem, w, h, layout="HWC")
        assert L.opsin_device(px, w, h, out.arg, GZ_SAMPLES_SRGB8) == 0
        out.check(expected_opsin(chk, fields.linear(rgb)), f"opsin image of a photo's bytes {w}x{h}")


# ------------------------------------------------------------------ 4. every way out ----
def case_every_way_out(L, mem, chk, dtype):
    """Every output layout x width of `dtype`, through all three entries -> the store paths taken."""
    paths = set()
    h = 16
    for w in OUT_WIDTHS[dtype]:
        lin0, lin1 = noise(w, h), noise(w, h, seed=1)
        em, edc = expected_mask(chk, lin0, lin1)
        p0, k0 = blc.pixels_of(mem, linear_source(lin0))
        p1, k1 = blc.pixels_of(mem, linear_source(lin1))
        for n, layout in enumerate(OUT_LAYOUTS):
            xyb, m, dc = Out(mem, w, h, dtype, layout), Out(mem, w, h, dtype, layout), Out(mem, w, h, dtype, OUT_LAYOUTS[(n + 1) % 4])
            L.opsin_device(p0, w, h, xyb.arg, GZ_SAMPLES_LINEAR)
            xyb.check(expected_opsin(chk, lin0), f"opsin image, {dtype} {layout} {w}")
            L.mask_device(p0, p1, w, h, m.arg, dc.arg, GZ_SAMPLES_LINEAR)
            m.check(em, f"mask, {dtype} {layout} {w}")
            dc.check(edc, f"mask_dc, {dtype} {w}")
            paths |= m.paths | dc.paths
            q, _ = quant_of(L, mem, linear_source(lin0), dtype=dtype, layout=QUANT_LAYOUTS[n])
            q.check(expected_quant(chk, lin0), f"quantisation field, {dtype} {QUANT_LAYOUTS[n]} {w}")
            paths |= q.paths
        # float32 mask beside a 16-bit mask_dc: two launches, one per type
        other = "bfloat16" if dtype == "float32" else "float32"
        m, dc = Out(mem, w, h, dtype, "CHW"), Out(mem, w, h, other, "HWC_crop")
        L.mask_device(p0, p1, w, h, m.arg, dc.arg, GZ_SAMPLES_LINEAR)
        m.check(em, f"mask, {dtype} beside {other}")
        dc.check(edc, f"mask_dc, {other} beside {dtype}")
    return paths


# ------------------------------------------------------------------ 5. every way in ----
def case_every_way_in(L, mem, chk, dtype):
    """The quantisation field from every layout and scale of the linear reader, at 17 x 16 -> the read paths taken."""
    paths = set()
    w, h = 17, 16
    rng = np.random.default_rng(w * 7 + len(dtype))
    base = (rng.random((h, w, 3), dtype=np.float32) * np.float32(255)).astype(np.float32)
    for scale in (1.0, 255.0):
        st = blc.to_storage(base / np.float32(scale), dtype)
        # (at 17 wide a contiguous image's rows start off the 16-byte grid: the crops inside a canvas keep the wide reads open)
        for layout in blc.LAYOUTS + ("HWC_crop", "CHW_crop"):
            src = dic.lay_out(st, dtype, layout)
            paths.add(blc.read_path(src))
            assert blc.rule(src.logical, dtype, scale)[1] == 0
            out, clamped = quant_of(L, mem, src, scale)
            out.check(expected_quant(chk, blc.planes_of(src.logical, dtype, scale)), f"quantisation field from {dtype} {layout} x{scale}")
            assert clamped == 0
    return paths


# ------------------------------------------------------------------ 6. clamp and count ----
def case_clamp_and_count(L, mem, chk):
    w, h = 17, 16
    for dtype in DTYPES:
        s0, n0 = blc.special_image(w, h, dtype, seed=3)
        s1, n1 = blc.special_image(w, h, dtype, seed=4)
        assert n0 >= 2 * blc.ALTERED and n1 >= 2 * blc.ALTERED
        lin0, lin1 = blc.planes_of(s0, dtype), blc.planes_of(s1, dtype)
        assert np.isfinite(lin0).all() and lin0.min() >= 0 and lin0.max() <= 255
        for layout in ("HWC", "CHW_crop_base1"):
            out, clamped = quant_of(L, mem, dic.lay_out(s0, dtype, layout))
            out.check(expected_quant(chk, lin0), f"quantisation field of the clamped planes, {dtype} {layout}")
            assert clamped == n0, (dtype, layout, clamped, n0)
            p0, k0 = blc.pixels_of(mem, dic.lay_out(s0, dtype, layout))
            p1, k1 = blc.pixels_of(mem, dic.lay_out(s1, dtype, layout))
            m, dc = Out(mem, w, h), Out(mem, w, h)
            assert L.mask_device(p0, p1, w, h, m.arg, dc.arg, GZ_SAMPLES_LINEAR) == n0 + n1     # (of both images)
            em, edc = expected_mask(chk, lin0, lin1)
            m.check(em, f"mask of the clamped images, {dtype} {layout}")
            dc.check(edc, f"mask_dc of the clamped images, {dtype} {layout}")
            assert L.mask_device(p0, None, w, h, m.arg, None, GZ_SAMPLES_LINEAR) == n0
            xyb = Out(mem, w, h)
            assert L.opsin_device(p1, w, h, xyb.arg, GZ_SAMPLES_LINEAR) == n1
            xyb.check(expected_opsin(chk, lin1), f"opsin image of the clamped planes, {dtype} {layout}")
