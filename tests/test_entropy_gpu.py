"""GPU: the device scan coder (gz_jpeg_histograms, gz_jpeg_scan*, k_scan_offsets) on the families, code tables and
shapes of tests/entropy_domain.py, against its reference coder, through the C ABI.  tests/test_entropy_domain.py pins
that coder to the writers and records which arm each case takes; the same cases run there through the emulation."""
import pytest

import entropy_domain as ed
import parity_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import guetzli_amd
    lib = guetzli_amd.load()
    assert lib.device_count() >= 1
    return lib


@pytest.fixture(scope="module")
def host():
    import guetzli_amd
    return guetzli_amd.load_host()


@pytest.fixture(scope="module")
def contexts(L):
    """One context per image size for the whole module: every family's frames and scans, of every layout and kind of
    table, follow each other on it."""
    cache = pc.ContextCache(L)
    yield cache
    cache.close()


@pytest.mark.parametrize("kind", ed.KINDS)
@pytest.mark.parametrize("family", list(ed.FAMILIES))
def test_entropy_domain(contexts, host, family, kind):
    """Statistics (templated and run-time-geometry kernel), scan bytes, bit and stuffed-byte counts, begin / end, and
    under the product's codes the whole file, at every shape of entropy_domain.SHAPES."""
    pc.case_entropy_domain(contexts, host, family, kind, ed.SHAPES)


def test_entropy_keep_across_scans(L, host):
    pc.case_entropy_keep_across_scans(L, host)


def test_scan_offsets_probe(L):
    """k_scan_offsets alone: see case_scan_probe -- which predecessors already hold an inclusive prefix when a tile
    looks back is a matter of timing here, the test cannot choose the arm; the long lengths run 20 times."""
    pc.case_scan_probe(L, repeats=20)
