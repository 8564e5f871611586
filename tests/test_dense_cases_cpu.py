"""The dense-counter cases on the CPU backend (GPUAGG_FLAG_CPU_BACKEND, Engine::aggregate): the
case tables of dense_cases.py, their inputs, references and restated geometry against the host
mirror, host-fed, no kernel names; "unaligned" columns are numpy views at offset 1.  The host
path has no LDS, lists or folds, so the flags only select the geometry that is restated and
asserted (for 256 workgroups).  Their GPU twins are in test_gpu_dense_cases.py."""

import pytest

from . import dense_cases as K

BE = K.Backend(None)


@pytest.fixture(scope="module", autouse=True)
def lib():
    from retina_amd import _abi, build
    build.build()
    return _abi.load()


@pytest.mark.parametrize("plan,flags,unaligned", K.PLAN_RUNS, ids=[K.plan_id(r) for r in K.PLAN_RUNS])
def test_plan_matrix(plan, flags, unaligned):
    K.plan_matrix(BE, plan, flags, unaligned)


@pytest.mark.parametrize("plan,which,unaligned,flags", K.SHAPE_RUNS,
                         ids=["%s-n%s-%s-f%d" % (p, n, "unaligned" if u else "aligned", f) for p, n, u, f in K.SHAPE_RUNS])
def test_launch_shape(plan, which, unaligned, flags):
    K.launch_shape(BE, plan, which, unaligned, flags)


@pytest.mark.parametrize("plan", K.SHAPE_PLANS)
def test_one_misaligned_column(plan):
    K.launch_shape(BE, plan, "4cu+3", "bytes", 0)


@pytest.mark.parametrize("case,flags", K.EDGE_RUNS, ids=["%s-f%d" % r for r in K.EDGE_RUNS])
def test_byte_edges(case, flags):
    K.byte_edges(BE, case, flags)


@pytest.mark.parametrize("flags", [0, K.PER_BATCH])
@pytest.mark.parametrize("tier", list(K.ONE_WINDOW))
def test_one_window(tier, flags):
    K.one_window(BE, tier, flags)


@pytest.mark.parametrize("flags", [0, K.PER_BATCH, K.NO_LDS_IP, K.NO_LDS_IP | K.PER_BATCH])
def test_partial_window(flags):
    K.partial_window(BE, flags)


@pytest.mark.parametrize("flags", [0, K.PER_BATCH])
@pytest.mark.parametrize("which", list(K.BOUNDARY))
def test_window_boundary(which, flags):
    K.window_boundary(BE, which, flags)


@pytest.mark.parametrize("flags,unaligned", [(0, False), (K.PER_BATCH, False), (0, True)],
                         ids=["f0", "f8", "f0-unaligned"])
def test_c5_no_rings(flags, unaligned):
    K.c5_no_rings(BE, flags, unaligned)


def test_exact_fold():
    K.exact_fold(BE)


@pytest.mark.parametrize("variant", list(K.HOT))
def test_hot_bin_per_batch(variant):
    K.hot_bin_per_batch(BE, variant)


@pytest.mark.parametrize("flags", [0, K.PER_BATCH])
@pytest.mark.parametrize("variant", list(K.HOT))
def test_hot_bin_deferred(variant, flags):
    K.hot_bin_deferred(BE, variant, flags)


@pytest.mark.parametrize("flags", [0, K.PER_BATCH])
@pytest.mark.parametrize("kind", ["hot", "uniform"])
def test_staged_rings(kind, flags):
    K.staged_rings(BE, kind, flags)


@pytest.mark.parametrize("flags", list(K.RING_FULL))
def test_ring_full(flags):
    K.ring_full(BE, flags)


@pytest.mark.parametrize("plan", K.STATE_PLANS)
def test_state_reset(plan):
    K.state_reset(BE, plan)


@pytest.mark.parametrize("plan", K.STATE_PLANS)
def test_state_relayout(plan):
    K.state_relayout(BE, plan)


@pytest.mark.parametrize("plan", K.STATE_PLANS)
def test_state_reconcile(plan):
    K.state_reconcile(BE, plan)


@pytest.mark.parametrize("plan", K.STATE_PLANS)
def test_state_double(plan):
    K.state_double(BE, plan)
