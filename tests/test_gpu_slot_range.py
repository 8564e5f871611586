"""The slot-range cases of slot_range_cases.py on the GPU: slot ids up to 2^21 - 2 through
every kernel that packs or indexes by them, the u16 limit of the LDS IP images, the HLL list
geometry at its row-count limits and the ABI's slot limits, with device-resident submits and
the kernels asserted by name.  Their CPU-backend twins are in test_slot_range_cpu.py."""

import pytest

from . import slot_range_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(gpu_device):
    return R.Backend(gpu_device)


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
