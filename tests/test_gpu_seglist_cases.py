"""Segment lists at their capacity and at the device-decided fold's threshold on the GPU
(wide_append, sparse_fold_wide_kernel's conditional fold and its counter reset, the compact
appends of aggregate_kernel and dense_local_kernel, sparse_fold_kernel, the fill clamps): the
cases of seglist_cases.py with device-resident submits and no sync() between them, every launch's
kernel asserted by name against the planner.  Their CPU-backend twins, which validate the
inputs, are in test_seglist_cases_cpu.py."""

import pytest

from . import seglist_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(gpu_device):
    return K.Backend(gpu_device)


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
