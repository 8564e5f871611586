"""Delta snapshots on the GPU (gpuagg_snapshot_delta: sparse_delta_kernel, dense_delta_kernel
and the rebase after a table rebuild): the cases of delta_cases.py with device-resident
submits.  Their CPU-backend twins are in test_delta_snapshot_cpu.py."""

import pytest

from retina_amd import workloads as W

from . import delta_cases as D
from .growth_inputs import PARITY

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(gpu_device):
    return D.Backend(gpu_device)


@pytest.mark.parametrize("name", PARITY)
def test_accumulation_across_specs(be, name):
    D.accumulation(be, name)


def test_only_what_changed(be):
    D.only_what_changed(be)


@pytest.mark.parametrize("name", ["local-all6", "c5-local"])
def test_idle(be, name):
    D.idle(be, name)


@pytest.mark.parametrize("direct", [False, True], ids=["lds-regrow", "direct-rehash"])
def test_growth_between_deltas_wide(be, direct):
    from retina_amd import _abi
    kernel = D.growth_between_deltas(be, "small-wide", 4, flags=_abi.FLAG_REGROW_DIRECT if direct else 0,
                                     sparse_capacity_log2=4, sparse_max_log2=20)
    assert kernel == ("sparse_rehash_direct_kernel" if direct else "sparse_regrow_kernel")


def test_growth_between_deltas_compact(be):
    D.growth_between_deltas(be, "compact", 3, sparse_capacity_log2=8, sparse_max_log2=22)


@pytest.mark.parametrize("spec,remote", [(W.C1_REMOTE, True), (W.LOCAL_FWD_DROP, False)], ids=["wide", "dense"])
def test_retire(be, spec, remote):
    D.retire(be, spec, remote)


def test_more_slots(be):
    D.more_slots(be)


@pytest.mark.parametrize("spec,remote", [(W.C1_REMOTE, True), (W.LOCAL_FWD_DROP, False)], ids=["wide", "dense"])
def test_reset_and_reconcile(be, spec, remote):
    D.reset_and_reconcile(be, spec, remote)


@pytest.mark.parametrize("name", ["local-c1-ip-ns-pod-wl", "remote-plain"])
def test_full_snapshots_between(be, name):
    D.full_snapshots_between(be, name)


@pytest.mark.parametrize("kw", [{}, dict(sparse_capacity_log2=4, sparse_max_log2=20)], ids=["fixed", "growing"])
def test_import(be, kw):
    D.imported(be, **kw)


def test_smallest_shapes(be):
    D.smallest_shapes(be)
