"""The sketch pass on the GPU at every depth, width, precision and scatter kernel
(launch_sketches, launch_sketch): the cases of sketch_cases.py with device-resident submits,
each asserting the scatter kernel it is there for by name.  Their CPU-backend twins are in
test_sketch_shapes_cpu.py."""

import pytest

from . import sketch_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(gpu_device):
    return K.Backend(gpu_device)


@pytest.mark.parametrize("d,flags", K.DEPTHS, ids=["d%d-f%d" % c for c in K.DEPTHS])
def test_depth_sweep(be, d, flags):
    K.depth_sweep(be, d, flags)


@pytest.mark.parametrize("d", [4, 3])
def test_cms_only(be, d):
    K.cms_only(be, d)


@pytest.mark.parametrize("p,n_pods", K.HLL_ONLY, ids=["p%d" % c[0] for c in K.HLL_ONLY])
def test_hll_only(be, p, n_pods):
    K.hll_only(be, p, n_pods)


@pytest.mark.parametrize("w", K.NARROW)
def test_narrow_rows(be, w):
    K.narrow_rows(be, w)


@pytest.mark.parametrize("flags", [0, K.CUCKOO], ids=["radix", "cuckoo"])
def test_rings_do_not_fit(be, flags):
    K.rings_do_not_fit(be, flags)


def test_rings_round2(be):
    K.rings_round2(be)


def test_direct_hll(be):
    K.direct_hll(be)


def test_direct_flag(be):
    K.direct_flag(be)


@pytest.mark.parametrize("d,flags", K.UNALIGNED, ids=["d%d-f%d" % c for c in K.UNALIGNED])
def test_unaligned(be, d, flags):
    K.unaligned(be, d, flags)


def test_mixed_accumulate(be):
    K.mixed_accumulate(be)


@pytest.mark.parametrize("unaligned", [False, True], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("which", K.RAGGED)
def test_ragged_n(be, which, unaligned):
    K.ragged_n(be, which, unaligned)


@pytest.mark.parametrize("unaligned", [False, True], ids=["aligned", "unaligned"])
def test_list_overflow(be, unaligned):
    K.list_overflow(be, unaligned)


@pytest.mark.parametrize("d", [1, 5, 16])
def test_cms_estimates(be, d):
    K.cms_estimates(be, d)


@pytest.mark.parametrize("p", [4, 18])
def test_hll_estimates(be, p):
    K.hll_estimates(be, p)
