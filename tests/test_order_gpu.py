"""GPU: the device side of phase B (gz_kernels_order.h through entry_phaseb.h) on the families of tests/order_domain.py,
against its restatements, through the C ABI and the hooks gz_probe_set_block_max / _set_search / _order_state.
tests/test_order_domain.py pins the restatements and records which arm each case takes; the same cases run there through
the emulation.  Bits and integers only: nothing here has a tolerance."""
import pytest

import order_domain as od
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
    """One context per (size, target, use) for the whole module: the cases follow each other on it."""
    cache = pc.TargetContexts(L)
    yield cache
    cache.close()


@pytest.mark.parametrize("target", od.TARGETS)
@pytest.mark.parametrize("gi", range(len(od.WEIGHT_GRIDS)))
@pytest.mark.parametrize("family", list(od.WEIGHT_FAMILIES))
def test_order_weights(contexts, family, gi, target):
    """k_block_max_group, k_weights_flag, k_weights_gather at every radius, direction and target_mul."""
    pc.case_order_weights(contexts, family, gi, target)


@pytest.mark.parametrize("family", od.ORDER_FAMILIES)
def test_order_build(contexts, family):
    """k_order_sizes / k_order_fill through all four entry points, the 16 900-block context included."""
    pc.case_order_build(contexts, family)


@pytest.mark.parametrize("family", od.ADVANCE_FAMILIES)
def test_order_advance(contexts, family):
    pc.case_order_advance(contexts, family)


@pytest.mark.parametrize("family", od.STEP_FAMILIES)
def test_order_steps(L, contexts, family):
    """k_apply_steps_hist + k_steps_hist_sum, k_apply_steps."""
    pc.case_order_steps(L, contexts, family)


@pytest.mark.parametrize("short", (False, True))
@pytest.mark.parametrize("per_block", od.PER_BLOCK)
def test_order_descent_position(contexts, per_block, short):
    pc.case_order_descent(contexts, per_block, big=False, short=short)


@pytest.mark.parametrize("short", (False, True))
@pytest.mark.parametrize("per_block", od.PER_BLOCK)
def test_order_descent_position_large(contexts, per_block, short):
    """Every blocks_to_change up to 16 900 whose product lands within one of a multiple of 10; the cut log and the
    rearranged order are compared at every 25th (a fetch of up to 338 000 entries from two contexts each)."""
    pc.case_order_descent(contexts, per_block, big=True, short=short, log_every=25)
