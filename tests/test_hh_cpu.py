"""The sketch-readout cases of hh_cases.py on the CPU backend (GPUAGG_FLAG_CPU_BACKEND: the
host loops of gpuagg_cpu.cpp after Engine::sketch), host-fed; "unaligned" columns are numpy
views at offset 1.  Their GPU twins are in test_gpu_hh.py."""

import pytest

from . import hh_cases as H
from . import sketch_cases as K

BE = K.Backend(None)


@pytest.fixture(scope="module", autouse=True)
def lib():
    from retina_amd import _abi, build
    build.build()
    return _abi.load()


@pytest.mark.parametrize("T", H.THRESHOLDS)
@pytest.mark.parametrize("w", H.WIDTHS)
def test_one_submit(w, T):
    H.one_submit(BE, w, T)


@pytest.mark.parametrize("T", H.THRESHOLDS)
@pytest.mark.parametrize("w", H.WIDTHS)
def test_three_submits(w, T):
    H.three_submits(BE, w, T)


def test_tie_order():
    H.tie_order(BE)


@pytest.mark.parametrize("unaligned", [False, True], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("which", H.RAGGED)
def test_ragged(which, unaligned):
    H.ragged(BE, which, unaligned)


@pytest.mark.parametrize("d", H.DEPTHS)
def test_depths(d):
    H.depths(BE, d)


def test_one_key_many_lanes():
    H.one_key_many_lanes(BE)


def test_table_full():
    H.table_full(BE)


def test_off_and_on():
    H.off_and_on(BE)


def test_add_candidates():
    H.add_candidates(BE)


def test_merge():
    H.merge(BE)


@pytest.mark.parametrize("p", H.HLL_P)
def test_hll_all(p):
    H.hll_all(BE, p)


def test_hll_growth():
    H.hll_growth(BE)
