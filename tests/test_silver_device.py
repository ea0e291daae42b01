"""Params::use_silver_screen on the device: gz_downsample_silver / gz_probe_silver_yuv420 (csrc/gz_kernels_silver.h)
against the host form of RGBToYUV420 (host/silver_screen.cc through gzh_silver_screen_yuv420) and against the
unmodified reference, bit for bit.

Every float of the conversion is static_cast<float>(pow(...)) of glibc's pow; the device evaluates its own pow together
with a proof that both round to the same float (gz_pow_to_float, csrc/gz_math.h) and hands the cells it cannot prove to
the library's host code.  The CPU part runs the same sources in the emulation, where pow IS libm's: the emulation's
hook gz_emu_set_pow_ulps moves the "device's" pow by double ulps, so that the guard has something to catch.  The GPU part
runs the real thing and measures how far the device's pow is from libm's.

Census of the CPU fields (host form, final state; counted before this list was fixed, CENSUS below): noise alone drives
both bounds of Clip in the decoded pixels, in the luma guess and in the chroma guesses at every size; the primaries
add hundreds of each; white / black / the checkers sit on the luma bounds with every sample.  33x35 has a last column
and a last row of one-pixel-wide cells (and the one-pixel corner cell), 34x33 a last row only, 100x84 neither."""
import ctypes as C
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import fields
import images
from checkers import assert_bits_equal, ref
from guetzli_amd import capi
from guetzli_amd.capi import GuetzliAmdError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu  # noqa: E402

needs_ref = pytest.mark.skipif(ref is None, reason="oracle/_ref/libgz_ref.so not built")
TARGET = 0.971769
FIELDS = ("noise", "primaries", "checker1", "checker8", "grey", "white", "black", "bees")
# Samples of the host form's FINAL state, summed over FIELDS: decoded pixel channels that left [0, 255] before Clip
# (rec_lo, rec_hi), luma guesses on a bound (y_lo, y_hi), chroma guesses on a bound (c_lo, c_hi).  From census() below.
CENSUS = {
    (33, 35): dict(rec_lo=899, rec_hi=376, y_lo=2317, y_hi=2310, c_lo=63, c_hi=188),
    (34, 33): dict(rec_lo=852, rec_hi=355, y_lo=2251, y_hi=2244, c_lo=55, c_hi=174),
    (100, 84): dict(rec_lo=5026, rec_hi=5297, y_lo=17935, y_hi=17894, c_lo=498, c_hi=776),
}


def field(name, w, h):
    if name == "bees":
        return np.ascontiguousarray(images.crop(w, h, 100, 60))
    return np.ascontiguousarray(fields.originals(w, h)[name])


class HostForm:
    """gzh_silver_screen_yuv420 of a host library: SilverScreenYUV420 with the host's libm, the yardstick.  Every
    (field, size) is computed once per library and shared."""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.gzh_silver_screen_yuv420.restype = C.c_int
        self.lib.gzh_silver_screen_yuv420.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self.cache = {}

    def planes(self, rgb):
        rgb = np.ascontiguousarray(rgb, np.uint8)
        h, w, _ = rgb.shape
        y, u, v = (np.zeros((h, w), np.float32) for _ in range(3))
        assert self.lib.gzh_silver_screen_yuv420(rgb.ctypes.data, w, h, y.ctypes.data, u.ctypes.data, v.ctypes.data) == 0
        return y, u, v

    def of_field(self, name, w, h):
        key = (name, w, h)
        if key not in self.cache:
            planes = self.planes(field(name, w, h))
            for p in planes:
                p.setflags(write=False)
            self.cache[key] = planes
        return self.cache[key]


def census(y, u, v):
    """Where the final state of the iteration meets Clip (numpy restatement of YUV420ToRGB on the returned planes)."""
    f32 = np.float32
    h, w = y.shape
    gu, gv = u[::2, ::2], v[::2, ::2]
    h2, w2 = gu.shape
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = yy // 2, xx // 2
    xn = np.clip(cx + np.where(xx & 1, 1, -1), 0, w2 - 1)
    yn = np.clip(cy + np.where(yy & 1, 1, -1), 0, h2 - 1)

    def fancy(g):
        return (f32(9) * g[cy, cx] + f32(3) * g[cy, xn] + f32(3) * g[yn, cx] + f32(1) * g[yn, xn]) / f32(16)
    fu, fv = fancy(gu), fancy(gv)
    rec = np.stack([y + f32(1.402) * (fv - f32(128)),
                    y - f32(0.344136) * (fu - f32(128)) - f32(0.714136) * (fv - f32(128)),
                    y + f32(1.772) * (fu - f32(128))])
    return dict(rec_lo=int((rec < 0).sum()), rec_hi=int((rec > 255).sum()), y_lo=int((y == 0).sum()), y_hi=int((y == 255).sum()),
                c_lo=int((gu == 0).sum() + (gv == 0).sum()), c_hi=int((gu == 255).sum() + (gv == 255).sum()))


def assert_planes_equal(got, exp, what):
    for g, e, name in zip(got, exp, "yuv"):
        assert_bits_equal(g, e, f"{what}: plane {name}")


# ------------------------------------------------------------------ CPU: the emulation ----
@pytest.fixture(scope="module")
def emu():
    L = capi.Library(build_emu.build())
    L.lib.gz_emu_set_pow_ulps.argtypes = [C.c_int]
    L.lib.gz_emu_fail_launch.argtypes = [C.c_long]
    L.lib.gz_emu_launch_calls.restype = C.c_long
    return L


@pytest.fixture(scope="module")
def host_emu():
    return HostForm(build_emu.build_host())


CPU_SIZES = [(33, 35), (34, 33), (100, 84)]


@pytest.mark.parametrize("wh", CPU_SIZES)
def test_the_fields_meet_every_clip_bound_and_edge_cell(host_emu, wh):
    """The census the module's docstring quotes, recomputed: what the plane tests below can see at all."""
    w, h = wh
    total = {}
    for name in FIELDS:
        for k, n in census(*host_emu.of_field(name, w, h)).items():
            total[k] = total.get(k, 0) + n
    print(wh, total)
    assert all(n > 0 for n in total.values()), total
    # (the recorded figures are this libm's; another one may move a sample across a bound, not halve a count)
    assert all(2 * total[k] >= n for k, n in CENSUS[wh].items()), (total, CENSUS[wh])
    assert all(n > 0 for n in census(*host_emu.of_field("noise", w, h)).values())
    # one-column and one-row cells: by the sizes' parity
    assert {(w & 1, h & 1) for w, h in CPU_SIZES} == {(1, 1), (0, 1), (0, 0)}


@pytest.mark.parametrize("guard_log2", [40, -1])
@pytest.mark.parametrize("wh", CPU_SIZES)
def test_planes_equal_the_host_form(emu, host_emu, wh, guard_log2):
    """guard_log2 = -1: every cell of every pass goes through gather, the host's libm and patch (1024 cells a chunk:
    100x84 has 2100 cells, three chunks, the last one partial; the small sizes one partial chunk)."""
    w, h = wh
    cells = ((w + 1) // 2) * ((h + 1) // 2)
    for name in FIELDS:
        y, u, v, cnt = emu.probe_silver_yuv420(field(name, w, h), guard_log2)
        assert_planes_equal((y, u, v), host_emu.of_field(name, w, h), f"{name} {w}x{h} guard {guard_log2}")
        assert cnt[0] == 21 * cells
        # (the guard judges the value, not the device: a power near a float rounding boundary goes to the host in the
        #  emulation too -- and a flat field whose one value is such a power goes there with every cell)
        assert cnt[1] == cnt[0] if guard_log2 < 0 else cnt[1] <= cnt[0], cnt


def test_the_guard_has_teeth(emu, host_emu):
    """The emulated device pow 1000 double ulps off libm's, either way (2^-42 relative: inside G = 2^-40): the planes are
    still the host's, and cells did go to the host.  The control: the same skew without the guard changes the planes."""
    w, h = 256, 192
    rgb = field("noise", w, h)
    exp = host_emu.of_field("noise", w, h)
    try:
        for skew in (1000, -1000):
            emu.lib.gz_emu_set_pow_ulps(skew)
            y, u, v, cnt = emu.probe_silver_yuv420(rgb, 40)
            assert_planes_equal((y, u, v), exp, f"skew {skew}")
            assert 0 < cnt[1] <= 0.005 * cnt[0], cnt
            print(f"skew {skew}: {cnt[1]} of {cnt[0]} cell-passes on the host")
        y, u, v, cnt = emu.probe_silver_yuv420(rgb, 64)   # (skew -1000, no guard)
        assert cnt[1] == 0
        differing = sum(int((a.view(np.uint32) != b.view(np.uint32)).sum()) for a, b in zip((y, u, v), exp))
        print(f"no guard: {differing} samples differ")
        assert differing > 0, "the skew changes nothing on this input: the test above proves nothing"
    finally:
        emu.lib.gz_emu_set_pow_ulps(0)


def test_fallback_share_is_small(emu, host_emu):
    """At the production guard about 19 * 2.4e-5 = 4.6e-4 of the cell-passes hold an unproven power; the cap is ten
    times that, and far below "everything quietly went to the host"."""
    _, _, _, cnt = emu.probe_silver_yuv420(field("noise", 100, 84), 40)
    print(f"{cnt[1]} of {cnt[0]} cell-passes on the host ({cnt[1] / cnt[0]:.2e})")
    assert 0 < cnt[1] <= 0.005 * cnt[0], cnt


def host_planes_of_original(ctx, host):
    """RGBToYUV420 of OutputImage::ToSRGB() of the unquantised original, on the host."""
    ctx.quantize(None, download=False)
    srgb, _ = ctx.reconstruct()
    return host.planes(srgb)


WHOLE_CALL = [(40, 32, 100, 60), (35, 33, 200, 100), (100, 84, 30, 40)]


def whole_call(L, host, case):
    """gz_downsample_silver's coefficients, and gz_downsample_planes' of the host form's planes."""
    w, h, x0, y0 = case
    rgb = np.ascontiguousarray(images.crop(w, h, x0, y0))
    with L.context(rgb, TARGET) as ctx:
        co = ctx.encode_rgb()
        got, cnt = ctx.downsample_silver()
        assert ctx.frame_layout()[0] == 2
    with L.context(rgb, TARGET) as ctx:
        ctx.encode_rgb(download=False)
        exp = ctx.downsample_planes(*host_planes_of_original(ctx, host))
    assert cnt[0] == 21 * ((w + 1) // 2) * ((h + 1) // 2)
    return co, got, exp, cnt


@pytest.mark.parametrize("case", WHOLE_CALL)
def test_downsample_silver_equals_downsample_planes_of_the_host_form(emu, host_emu, case):
    try:
        emu.lib.gz_emu_set_pow_ulps(-7)   # (a "device" pow that is not libm's)
        _, got, exp, _ = whole_call(emu, host_emu, case)
    finally:
        emu.lib.gz_emu_set_pow_ulps(0)
    assert_bits_equal(got, exp, "gz_downsample_silver against gz_downsample_planes(host form)")


@needs_ref
@pytest.mark.parametrize("case", WHOLE_CALL)
def test_downsample_silver_equals_the_reference(emu, host_emu, case):
    w, h = case[:2]
    co, got, _, _ = whole_call(emu, host_emu, case)
    assert_bits_equal(got, ref.downsample(co, w, h, silver=True), "gz_downsample_silver against OutputImage::Downsample")


def test_launch_failures_leave_no_original(emu):
    """A launch failing anywhere inside gz_downsample_silver: GZ_E_HIP, the frame stays 4:4:4, the half-written
    original is not quantized, and the next Compare is that of a fresh context (patch_reconstruct = 2: a Compare that
    trusts kept planes checks them itself) -- as after a failed gz_downsample_planes."""
    rgb = np.ascontiguousarray(images.crop(40, 32, 100, 60))
    q = np.full((3, 64), 3, np.int32)

    def setup():
        ctx = emu.context(rgb, TARGET)
        ctx.set_config(patch_reconstruct=2)
        ctx.encode_rgb(download=False)
        ctx.quantize(q, download=False)
        ctx.compare()
        return ctx
    ctx = setup()
    before = emu.lib.gz_emu_launch_calls()
    ctx.downsample_silver(download=False)
    n_launches = emu.lib.gz_emu_launch_calls() - before
    ctx.close()
    assert n_launches >= 1 + 21 * 2 + 1 + 3, n_launches   # ToSRGB, 21 passes and their gathers, the upsample, three components
    for n in range(n_launches):
        ctx = setup()
        emu.lib.gz_emu_fail_launch(n)
        try:
            with pytest.raises(GuetzliAmdError, match="GZ_E_HIP"):
                ctx.downsample_silver(download=False)
        finally:
            emu.lib.gz_emu_fail_launch(-1)
        assert ctx.frame_layout()[0] == 1, n
        got = ctx.compare()
        with emu.context(rgb, TARGET) as fresh:
            fresh.set_coeffs(ctx.get_coeffs())
            exp = fresh.compare()
        for g, e, what in zip(got, exp, ("distance", "distance map", "block maxima")):
            assert_bits_equal(np.asarray(g, np.float32), np.asarray(e, np.float32), f"launch {n}: {what}")
        co = ctx.get_coeffs()
        with pytest.raises(GuetzliAmdError, match="GZ_E_STATE"):
            ctx.quantize(q)
        assert np.array_equal(ctx.get_coeffs(), co), f"launch {n} failed, and a half-written original was quantized"
        ctx.close()


def test_bad_arguments(emu):
    z = np.zeros(3 * 64, np.float32)
    lib = emu.lib
    assert lib.gz_downsample_silver(None, None, None) == -1
    assert lib.gz_probe_silver_yuv420(0, None, 8, 8, 40, z.ctypes.data, z.ctypes.data, z.ctypes.data, None) == -1
    assert lib.gz_probe_silver_yuv420(0, z.ctypes.data, 0, 8, 40, z.ctypes.data, z.ctypes.data, z.ctypes.data, None) == -1
    assert lib.gz_probe_silver_yuv420(0, z.ctypes.data, 8, 8, 65, z.ctypes.data, z.ctypes.data, z.ctypes.data, None) == -1
    assert lib.gz_probe_silver_yuv420(0, z.ctypes.data, 8, 8, -2, z.ctypes.data, z.ctypes.data, z.ctypes.data, None) == -1
    rgb = np.ascontiguousarray(images.crop(40, 32, 100, 60))
    with emu.context(rgb, TARGET) as ctx:
        with pytest.raises(GuetzliAmdError, match="GZ_E_STATE"):   # no original coefficients yet
            ctx.downsample_silver()
        ctx.encode_rgb(download=False)
        ctx.downsample_silver(download=False)
        with pytest.raises(GuetzliAmdError, match="GZ_E_STATE"):   # a 4:2:0 frame
            ctx.downsample_silver()


def test_encoder_reports_the_cell_rounds(emu):
    """A whole use_silver_screen encode through the emulation: the driver calls gz_downsample_silver and reports its
    counters."""
    from guetzli_amd.encoder import HostLibrary
    host = HostLibrary(build_emu.build_host())
    rgb = np.ascontiguousarray(images.crop(40, 32, 100, 60))
    jpg, info = host.process(rgb, quality=95.0, force_420=True, use_silver_screen=True)
    assert info["counters"]["silver screen cell rounds"] == 21 * 20 * 16
    assert 0 <= info["counters"]["silver screen cell rounds on host"] <= 21 * 20 * 16 // 50
    assert "downsample" in info["timers"]
    if ref is not None:
        exp, _ = ref.process_params(rgb, ref._butteraugli_score_for_quality(95.0), force_420=True, silver=True)
        assert jpg == exp


def test_guarded_pow_on_the_host(tmp_path):
    """tests/cpp/silver_guard.cc: gz_pow_to_float against libm over a strided sweep of the float arguments of both
    exponents, with the emulated device pow -1000, 0 and +1000 ulps off; built with the host sanitizers as a plain
    program."""
    exe = str(tmp_path / "silver_guard")
    subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-DGZ_EMU", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "guetzli_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "tests", "emu"), os.path.join(ROOT, "tests", "cpp", "silver_guard.cc"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count(" 0 mismatches") == 6 and "every unambiguous result is libm's" in out.stdout


# ------------------------------------------------------------------------ GPU ----
@pytest.fixture(scope="module")
def gpu():
    import guetzli_amd
    return guetzli_amd.load()


@pytest.fixture(scope="module")
def host_gpu():
    from guetzli_amd import build as gzbuild
    gzbuild.build()
    return HostForm(gzbuild.build_host())


def libm_pow(base, expo):
    """pow of the C library, element by element (numpy's own loops may use another implementation)."""
    return np.fromiter(map(math.pow, base.tolist(), itertools.repeat(expo)), np.float64, base.size)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["gamma_to_linear", "linear_to_gamma"])
def test_device_pow_is_close_to_libm_and_the_guard_holds(gpu, which):
    """The device's FP64 pow against the host's on 2^20 arguments per exponent -- log-uniform in [2^-30, 1] and
    bytes' worth of uniform ones in [0, 255] / 255 -- : within relative 2^-44 (16 times inside G = 2^-40, 256 double
    ulps, where the documented accuracy is single digits), and every float the guard does not call ambiguous is libm's."""
    rng = np.random.default_rng(20261018)
    n = 1 << 19
    log_uniform = np.exp2(rng.uniform(-30.0, 0.0, n)).astype(np.float32)
    uniform = (rng.uniform(0.0, 255.0, n).astype(np.float32) / np.float32(255.0)).astype(np.float32)
    base = np.concatenate([log_uniform, uniform, np.float32([0.0, 1.0])]).astype(np.float64)
    expo, scale = (2.2, 1.0) if which == "gamma_to_linear" else (1.0 / 2.2, 255.0)
    p_dev, f_dev, amb = gpu.probe_math(17, base, p=(expo, scale), outs=3)
    p_host = libm_pow(base, expo)
    want = (scale * p_host).astype(np.float32)
    rel = np.abs(p_dev - p_host) / np.maximum(p_host, np.finfo(np.float64).tiny)
    clear = amb == 0.0
    wrong = int((f_dev.astype(np.float32).view(np.uint32) != want.view(np.uint32))[clear].sum())
    print(f"{which}: largest relative difference {rel.max():.3e} = {rel.max() * 2.0 ** 52:.2f} double ulps of 1; "
          f"{int((~clear).sum())} of {base.size} ambiguous ({(~clear).mean():.2e}); {wrong} unambiguous floats differ")
    assert rel.max() <= 2.0 ** -44, rel.max()
    assert wrong == 0
    assert (~clear).mean() < 1e-3
    assert clear[-2:].all() and f_dev[-2] == 0.0 and f_dev[-1] == scale   # pow(0, y), pow(1, y): exact, never ambiguous


GPU_SIZES = [(33, 35), (100, 84), (255, 193)]


@pytest.mark.gpu
@pytest.mark.parametrize("guard_log2", [40, -1])
@pytest.mark.parametrize("wh", GPU_SIZES)
def test_gpu_planes_equal_the_host_form(gpu, host_gpu, wh, guard_log2):
    w, h = wh
    cells = ((w + 1) // 2) * ((h + 1) // 2)
    on_host = evaluated = 0
    for name in FIELDS:
        y, u, v, cnt = gpu.probe_silver_yuv420(field(name, w, h), guard_log2)
        assert_planes_equal((y, u, v), host_gpu.of_field(name, w, h), f"{name} {w}x{h} guard {guard_log2}")
        assert cnt[0] == 21 * cells
        if guard_log2 < 0:
            assert cnt[1] == cnt[0]
        elif name == "noise":
            assert cnt[1] <= 0.005 * cnt[0], cnt   # the fallback cap
        evaluated += cnt[0]
        on_host += cnt[1]
    print(f"{w}x{h} guard {guard_log2}: {on_host} of {evaluated} cell-passes on the host ({on_host / evaluated:.2e})")


@pytest.mark.gpu
@pytest.mark.parametrize("case", WHOLE_CALL[1:])
def test_gpu_downsample_silver_equals_the_reference(gpu, host_gpu, case):
    w, h = case[:2]
    co, got, exp, cnt = whole_call(gpu, host_gpu, case)
    assert_bits_equal(got, exp, "gz_downsample_silver against gz_downsample_planes(host form)")
    assert ref is not None, "oracle/_ref/libgz_ref.so is missing"
    assert_bits_equal(got, ref.downsample(co, w, h, silver=True), "gz_downsample_silver against OutputImage::Downsample")
    assert cnt[1] <= 0.005 * cnt[0], cnt


@pytest.mark.gpu
def test_gpu_encoder_reports_the_cell_rounds():
    import guetzli_amd
    rgb = np.ascontiguousarray(images.crop(100, 84, 30, 40))
    _, info = guetzli_amd.process(rgb, quality=95.0, force_420=True, use_silver_screen=True)
    assert info["counters"]["silver screen cell rounds"] == 21 * 50 * 42
    assert info["counters"]["silver screen cell rounds on host"] <= 0.005 * 21 * 50 * 42
