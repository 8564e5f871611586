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


def test_hash_slices():
    """hh_cases' numpy restatement of cms_base and its three slices (table home, tag, LDS-set
    home) against tests/hh_hash_test.cpp, which prints what the kernels compute: 4,096 random
    keys, and every key the table cases choose by these slices."""
    import numpy as np
    keys, base = H.pool()
    fixtures = np.concatenate([np.concatenate(H.twins(lg)[:n]) for lg, n in H.TWINS.items()]
                              + [np.flatnonzero(H.home(base[:8192], 4) == H.CHAIN_HOME)[:19],
                                 H.groups_of(H.lds_home(base[:100_000]), 6)[0][:6]])
    some = np.random.default_rng(79).integers(0, 2**32, (4096, 4), dtype=np.uint64).astype(np.uint32)
    for k in (some, keys[fixtures]):
        got, b = H.host_slices(k), H.cms_base(k)
        assert np.array_equal(got[:, 0], b)
        assert np.array_equal(got[:, 1].astype(np.int64), H.home(b, 32))
        assert np.array_equal(got[:, 2].astype(np.int64), H.tag(b))
        assert np.array_equal(got[:, 3].astype(np.int64), H.lds_home(b))
    assert np.array_equal(H.cms_base(keys[fixtures]), base[fixtures])


def test_pool_groups():
    """What the table cases need of the key pool (and what it holds)."""
    _, base = H.pool()
    found = {lg: len(H.twins(lg)) for lg in (4, 8, 0)}
    per_home = max(len(r) for r in H.groups_of(H.lds_home(base[:100_000]), 6))
    print("groups sharing tag and home: %d (16 slots), %d (256 slots); a tag alone: %d; keys per LDS-set home <= %d"
          % (found[4], found[8], found[0], per_home))
    assert found[4] >= 4 and found[8] >= 8 and per_home >= 6


@pytest.mark.parametrize("through", ["add", "records"])
def test_same_home_chain(through):
    H.same_home_chain(BE, through)


@pytest.mark.parametrize("through", ["add", "records"])
@pytest.mark.parametrize("lg", sorted(H.TWINS))
def test_tag_twins(lg, through):
    H.tag_twins(BE, lg, through)


def test_lds_six():
    H.lds_six(BE)


def test_lds_overflow():
    H.lds_overflow(BE)


def test_zero_estimates():
    H.zero_estimates(BE)


def test_largest_table():
    H.largest_table(BE)


def test_direct_rows():
    H.direct_rows(BE)


def test_capacity_reports():
    H.capacity_reports(BE)


@pytest.mark.parametrize("p", H.HLL_SWEEP)
def test_hll_sweep(p):
    H.hll_sweep(BE, p)


@pytest.mark.parametrize("p", sorted(H.HIGH_RANK))
def test_hll_high_ranks(p):
    H.hll_high_ranks(BE, p)
