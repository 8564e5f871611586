"""The segment-list cases of seglist_cases.py on the CPU backend (GPUAGG_FLAG_CPU_BACKEND).  That
backend has no lists, so these tests do not exercise the paths the cases are named for: they
validate what the GPU twins (test_gpu_seglist_cases.py) rely on -- the inputs, every reference
(the host mirror driven through the same calls has to give it), the fills of every case against
the real planner's geometry for 64, 256 and 304 CUs, and the numpy restatement of the key
hashes against the engine's header."""

import numpy as np
import pytest

from . import seglist_cases as K


@pytest.fixture(scope="module")
def be():
    return K.Backend(None, 256)


def test_key_hash_restatement():
    """fmix64 / key_hash / the compact hash in numpy against tests/key_hash_test.cpp: every probed
    key of the two-group spec, the compact keys of one plan, and edge and random words."""
    rng = np.random.default_rng(5)
    p, c = K.pool("two"), K.compact_pool("dns-only")
    edge = np.array([[0, 0, 0], [(1 << 64) - 1] * 3, [1 << 63, 0, 1], [0, 1 << 63, (1 << 32) - 1]], np.uint64)
    compact = np.stack([c.key, np.zeros_like(c.key), np.zeros_like(c.key)], 1)
    keys = np.concatenate([p.keys.reshape(-1, 3), compact, edge, rng.integers(0, 1 << 64, (2000, 3), dtype=np.uint64)])
    assert len(keys) >= 1000
    wide, comp = K.host_hashes(keys)
    assert (K.key_hash(keys[:, 0], keys[:, 1], keys[:, 2]) == wide).all()
    assert (K.compact_hash(keys[:, 0]) == comp).all()
    assert (K.fmix64(keys[:, 0] ^ K.SEED) == comp).all()


@pytest.mark.parametrize("spec_id", ["two", "four"])
def test_wide_pool(spec_id):
    """Both segments hold every kind of flow the cases pick, more than POOL_FLOWS of each."""
    p = K.pool(spec_id)
    kinds = {"two": [(0, 1), (1, 0)], "four": [(0, 2), (1, 1), (2, 0)]}[spec_id]
    assert sorted(p.kinds) == kinds and all(len(p.kinds[k]) == K.POOL_FLOWS[spec_id] for k in kinds)
    assert (p.vec.sum(1) == K.UPDATES[spec_id]).all()


@pytest.mark.parametrize("plan", K.COMPACT_PLANS)
def test_compact_pool(plan):
    """Every segment of the table has a key, the busiest several."""
    p = K.compact_pool(plan)
    assert len(p.of_segment(p.busiest(2)[1])) >= 4
    assert len(set(p.seg.tolist())) > K.COMPACT_SEGS // 2


@pytest.mark.parametrize("case,variant,spec_id", K.WIDE_RUNS, ids=[K.run_id(r) for r in K.WIDE_RUNS])
def test_wide(be, case, variant, spec_id):
    K.WIDE_CASES[case](be, variant, spec_id)


@pytest.mark.parametrize("op,variant", K.OP_RUNS, ids=[K.run_id(r) for r in K.OP_RUNS])
def test_wide_operation_under_a_kept_list(be, op, variant):
    K.WIDE_OPS[op](be, variant)


@pytest.mark.parametrize("case,plan,unaligned", K.COMPACT_RUNS, ids=[K.run_id(r) for r in K.COMPACT_RUNS])
def test_compact(be, case, plan, unaligned):
    K.COMPACT_CASES[case](be, plan, unaligned)


@pytest.mark.parametrize("unaligned", [False, True], ids=["aligned", "unaligned"])
def test_compact_two_hot_segments(be, unaligned):
    K.compact_two_hot(be, unaligned)


# ---- the fills against the planner on other CU counts (no engine: inputs and geometry only) ----
OTHER_CUS = [64, 304]
DRY_WIDE = [r for r in K.WIDE_RUNS if r[1] in K.GEOMETRY_VARIANTS]


@pytest.mark.parametrize("cus", OTHER_CUS)
@pytest.mark.parametrize("case,variant,spec_id", DRY_WIDE, ids=[K.run_id(r) for r in DRY_WIDE])
def test_wide_fills_on_other_devices(cus, case, variant, spec_id):
    K.WIDE_CASES[case](K.Backend(None, cus, dry=True), variant, spec_id)


@pytest.mark.parametrize("cus", OTHER_CUS)
@pytest.mark.parametrize("case,plan", [(c, p) for c in K.COMPACT_CASES for p in ("dns-two", "c5-staged")])
def test_compact_fills_on_other_devices(cus, case, plan):
    K.COMPACT_CASES[case](K.Backend(None, cus, dry=True), plan, False)
