"""The slot-range cases of slot_range_cases.py on GPUAGG_FLAG_CPU_BACKEND: their inputs and
references proven with no GPU (the kernel-name assertions are the GPU module's,
test_gpu_slot_range.py).  The two full-range functions intern 2^21 - 1 slots each and take
tens of seconds; everything else is small."""

import pytest

from . import slot_range_cases as R


@pytest.fixture(scope="module")
def be():
    return R.Backend(None)


def test_full_range_remote(be):
    R.full_range_remote(be)


def test_full_range_local(be):
    R.full_range_local(be)


@pytest.mark.parametrize("plan", list(R.U16_PLANS))
def test_u16_limit(be, plan):
    R.u16_limit(be, plan)


def test_u16_retire_reuse(be):
    R.u16_retire_reuse(be)


@pytest.mark.parametrize("which", list(R.HLL_ROWS))
def test_hll_row_limits(be, which):
    R.hll_row_limits(be, which)


def test_hll_list_overflow(be):
    R.hll_list_overflow(be)


def test_abi_max_slots(be):
    R.abi_max_slots(be)


def test_abi_capacity_and_reuse(be):
    R.abi_capacity_and_reuse(be)


def test_abi_refused_endpoints(be):
    R.abi_refused_endpoints(be)
