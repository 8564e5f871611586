"""The sketch-shape cases on the CPU backend (GPUAGG_FLAG_CPU_BACKEND, Engine::sketch): the
case tables of sketch_cases.py and the numpy restatement against the host mirror, host-fed,
no kernel names; "unaligned" columns are numpy views at offset 1.  The host path has no
lists, so the two overflow cases check the list-sizing arithmetic for 256 workgroups and
then the state.  Their GPU twins are in test_gpu_sketch_shapes.py."""

import pytest

from . import sketch_cases as K

BE = K.Backend(None)


@pytest.fixture(scope="module", autouse=True)
def lib():
    from retina_amd import _abi, build
    build.build()
    return _abi.load()


@pytest.mark.parametrize("d,flags", K.DEPTHS, ids=["d%d-f%d" % c for c in K.DEPTHS])
def test_depth_sweep(d, flags):
    K.depth_sweep(BE, d, flags)


@pytest.mark.parametrize("d", [4, 3])
def test_cms_only(d):
    K.cms_only(BE, d)


@pytest.mark.parametrize("p,n_pods", K.HLL_ONLY, ids=["p%d" % c[0] for c in K.HLL_ONLY])
def test_hll_only(p, n_pods):
    K.hll_only(BE, p, n_pods)


@pytest.mark.parametrize("w", K.NARROW)
def test_narrow_rows(w):
    K.narrow_rows(BE, w)


@pytest.mark.parametrize("flags", [0, K.CUCKOO], ids=["radix", "cuckoo"])
def test_rings_do_not_fit(flags):
    K.rings_do_not_fit(BE, flags)


def test_rings_round2():
    K.rings_round2(BE)


def test_direct_hll():
    K.direct_hll(BE)


def test_direct_flag():
    K.direct_flag(BE)


@pytest.mark.parametrize("d,flags", K.UNALIGNED, ids=["d%d-f%d" % c for c in K.UNALIGNED])
def test_unaligned(d, flags):
    K.unaligned(BE, d, flags)


def test_mixed_accumulate():
    K.mixed_accumulate(BE)


@pytest.mark.parametrize("unaligned", [False, True], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("which", K.RAGGED)
def test_ragged_n(which, unaligned):
    K.ragged_n(BE, which, unaligned)


@pytest.mark.parametrize("unaligned", [False, True], ids=["aligned", "unaligned"])
def test_list_overflow(unaligned):
    K.list_overflow(BE, unaligned)


@pytest.mark.parametrize("d", [1, 5, 16])
def test_cms_estimates(d):
    K.cms_estimates(BE, d)


@pytest.mark.parametrize("p", [4, 18])
def test_hll_estimates(p):
    K.hll_estimates(BE, p)
