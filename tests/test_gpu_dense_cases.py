"""The dense counters on the GPU in every kernel variant, residency and spill edge
(launch_aggregate: dense_lds_kernel, dense_local_kernel, spill_window_kernel,
stage_reduce_kernel): the cases of dense_cases.py with device-resident submits, each asserting
the kernel it is there for by name.  Their CPU-backend twins are in test_dense_cases_cpu.py."""

import pytest

from . import dense_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(gpu_device):
    return K.Backend(gpu_device)


@pytest.mark.parametrize("plan,flags,unaligned", K.PLAN_RUNS, ids=[K.plan_id(r) for r in K.PLAN_RUNS])
def test_plan_matrix(be, plan, flags, unaligned):
    K.plan_matrix(be, plan, flags, unaligned)


@pytest.mark.parametrize("plan,which,unaligned,flags", K.SHAPE_RUNS,
                         ids=["%s-n%s-%s-f%d" % (p, n, "unaligned" if u else "aligned", f) for p, n, u, f in K.SHAPE_RUNS])
def test_launch_shape(be, plan, which, unaligned, flags):
    K.launch_shape(be, plan, which, unaligned, flags)


@pytest.mark.parametrize("plan", K.SHAPE_PLANS)
def test_one_misaligned_column(be, plan):
    K.launch_shape(be, plan, "4cu+3", "bytes", 0)


@pytest.mark.parametrize("case,flags", K.EDGE_RUNS, ids=["%s-f%d" % r for r in K.EDGE_RUNS])
def test_byte_edges(be, case, flags):
    K.byte_edges(be, case, flags)


@pytest.mark.parametrize("flags", [0, K.PER_BATCH])
@pytest.mark.parametrize("tier", list(K.ONE_WINDOW))
def test_one_window(be, tier, flags):
    K.one_window(be, tier, flags)


@pytest.mark.parametrize("flags", [0, K.PER_BATCH, K.NO_LDS_IP, K.NO_LDS_IP | K.PER_BATCH])
def test_partial_window(be, flags):
    K.partial_window(be, flags)


@pytest.mark.parametrize("flags", [0, K.PER_BATCH])
@pytest.mark.parametrize("which", list(K.BOUNDARY))
def test_window_boundary(be, which, flags):
    K.window_boundary(be, which, flags)


@pytest.mark.parametrize("flags,unaligned", [(0, False), (K.PER_BATCH, False), (0, True)],
                         ids=["f0", "f8", "f0-unaligned"])
def test_c5_no_rings(be, flags, unaligned):
    K.c5_no_rings(be, flags, unaligned)


def test_exact_fold(be):
    K.exact_fold(be)


@pytest.mark.parametrize("variant", list(K.HOT))
def test_hot_bin_per_batch(be, variant):
    K.hot_bin_per_batch(be, variant)


@pytest.mark.parametrize("flags", [0, K.PER_BATCH])
@pytest.mark.parametrize("variant", list(K.HOT))
def test_hot_bin_deferred(be, variant, flags):
    K.hot_bin_deferred(be, variant, flags)


@pytest.mark.parametrize("flags", [0, K.PER_BATCH])
@pytest.mark.parametrize("kind", ["hot", "uniform"])
def test_staged_rings(be, kind, flags):
    K.staged_rings(be, kind, flags)


@pytest.mark.parametrize("flags", list(K.RING_FULL))
def test_ring_full(be, flags):
    K.ring_full(be, flags)


@pytest.mark.parametrize("plan", K.STATE_PLANS)
def test_state_reset(be, plan):
    K.state_reset(be, plan)


@pytest.mark.parametrize("plan", K.STATE_PLANS)
def test_state_relayout(be, plan):
    K.state_relayout(be, plan)


@pytest.mark.parametrize("plan", K.STATE_PLANS)
def test_state_reconcile(be, plan):
    K.state_reconcile(be, plan)


@pytest.mark.parametrize("plan", K.STATE_PLANS)
def test_state_double(be, plan):
    K.state_double(be, plan)
