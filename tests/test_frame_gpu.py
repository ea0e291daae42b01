"""GPU: the frame path (k_encode_rgb, k_quantize, k_reconstruct, k_reconstruct_listed, k_chroma_samples + k_reconstruct420,
k_to_float_pixels, k_set_downsampled_coeffs, the k_pp_* kernels) on the families of tests/frame_domain.py, against the
oracle, through the C ABI.  tests/test_frame_domain.py records which arm each family takes and runs the same cases through
the emulation.  Bits and integers only: nothing here has a tolerance."""
import pytest

import frame_domain as fd
import parity_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import guetzli_amd
    lib = guetzli_amd.load()
    assert lib.device_count() >= 1
    return lib


@pytest.fixture(scope="module")
def contexts(L):
    """One context per size for the whole module: the cases follow each other on it."""
    cache = pc.TargetContexts(L)
    yield cache
    cache.close()


def test_frame_encode(L, contexts):
    """k_encode_rgb: the colour lattice, checkerboards of primaries, one and seven replicated columns / rows."""
    pc.case_frame_encode(L, contexts, fd.PIXEL_SIZES + fd.FREE_SIZES + fd.CTX_SIZES[:9])


def test_frame_planes(L):
    """k_set_downsampled_coeffs: every factor pair, the source clamps, the rounding ties."""
    pc.case_frame_planes(L)


def test_frame_free_sizes(L):
    """k_to_float_pixels and gz_decode_coeffs (both chroma factors) below 8 pixels."""
    pc.case_frame_free_sizes(L)


@pytest.mark.parametrize("wh", fd.CTX_SIZES)
def test_frame_coeffs444(L, contexts, wh):
    """k_quantize, k_reconstruct, k_scatter_blocks and k_reconstruct_listed on every coefficient family and table."""
    for family in fd.COEFF_FAMILIES:
        pc.case_frame_coeffs444(L, contexts, *wh, family)


@pytest.mark.parametrize("wh", fd.CTX_SIZES)
def test_frame_coeffs420(L, contexts, wh):
    """k_quantize with the 4:2:0 component boundaries, k_chroma_samples + k_reconstruct420, gz_decode_coeffs factor 2."""
    for family in fd.COEFF_FAMILIES:
        pc.case_frame_coeffs420(L, contexts, *wh, family)


@pytest.mark.parametrize("wh", fd.CTX_SIZES)
def test_frame_downsample(L, contexts, wh):
    """gz_downsample: the k_pp_* kernels on the YUV fields, frames without a convolution interior among the sizes."""
    pc.case_frame_downsample(L, contexts, *wh)


@pytest.mark.parametrize("wh", fd.CTX_SIZES)
def test_frame_idct_copies(L, contexts, wh):
    """The copies of the integer IDCT against each other on the extreme luma blocks."""
    pc.case_frame_idct_copies(L, contexts, *wh)


@pytest.mark.parametrize("wh,per", [((139, 8000), 2), ((272, 8000), 4)])
def test_frame_strip_loop(L, wh, per):
    """k_reconstruct's strip loop as stage_reconstruct chooses it: strips of 8 blocks per workgroup, 4 halved while the
    grid has fewer than 2000 workgroups.
    139 x 8000: bw 18, three strips, bh 1000: per 4 gives 1000 workgroups, per 2 gives 2000 -> 2; two groups per block
    row, the second of one strip (the short last group); the last strip holds blocks 16 and 17 only; the row pitch 139
    is odd (scalar stores).
    272 x 8000: bw 34, five strips: per 4 gives 1000 * 2 = 2000 workgroups -> 4; the second group holds one strip; row
    pitch 272 (16-byte stores)."""
    assert pc.recon_strips_per_workgroup(*wh) == per
    pc.case_frame_strips(L, *wh)
