"""The sketch-readout cases of hh_cases.py on the GPU: hh_candidate_kernel behind every
device-resident submit, hh_rank_kernel and the readout kernels behind heavy_hitters /
hh_candidates / hh_info, hll_estimate_kernel behind hll_estimates (gpuagg_hh.hip).  Their
CPU-backend twins are in test_hh_cpu.py."""

import pytest

from . import hh_cases as H
from . import sketch_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(gpu_device):
    return K.Backend(gpu_device)


@pytest.mark.parametrize("T", H.THRESHOLDS)
@pytest.mark.parametrize("w", H.WIDTHS)
def test_one_submit(be, w, T):
    H.one_submit(be, w, T)


@pytest.mark.parametrize("T", H.THRESHOLDS)
@pytest.mark.parametrize("w", H.WIDTHS)
def test_three_submits(be, w, T):
    H.three_submits(be, w, T)


def test_tie_order(be):
    H.tie_order(be)


@pytest.mark.parametrize("unaligned", [False, True], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("which", H.RAGGED)
def test_ragged(be, which, unaligned):
    H.ragged(be, which, unaligned)


@pytest.mark.parametrize("d", H.DEPTHS)
def test_depths(be, d):
    H.depths(be, d)


def test_one_key_many_lanes(be):
    H.one_key_many_lanes(be)


def test_table_full(be):
    H.table_full(be)


def test_off_and_on(be):
    H.off_and_on(be)


def test_add_candidates(be):
    H.add_candidates(be)


def test_merge(be):
    H.merge(be)


@pytest.mark.parametrize("p", H.HLL_P)
def test_hll_all(be, p):
    H.hll_all(be, p)


def test_hll_growth(be):
    H.hll_growth(be)


@pytest.mark.parametrize("through", ["add", "records"])
def test_same_home_chain(be, through):
    H.same_home_chain(be, through)


@pytest.mark.parametrize("through", ["add", "records"])
@pytest.mark.parametrize("lg", sorted(H.TWINS))
def test_tag_twins(be, lg, through):
    H.tag_twins(be, lg, through)


def test_lds_six(be):
    H.lds_six(be)


def test_lds_overflow(be):
    H.lds_overflow(be)


def test_zero_estimates(be):
    H.zero_estimates(be)


def test_largest_table(be):
    H.largest_table(be)


def test_direct_rows(be):
    H.direct_rows(be)


def test_capacity_reports(be):
    H.capacity_reports(be)


@pytest.mark.parametrize("p", H.HLL_SWEEP)
def test_hll_sweep(be, p):
    H.hll_sweep(be, p)


@pytest.mark.parametrize("p", sorted(H.HIGH_RANK))
def test_hll_high_ranks(be, p):
    H.hll_high_ranks(be, p)
