"""Delta snapshots on the CPU backend (gpuagg_snapshot_delta, GPUAGG_FLAG_CPU_BACKEND):
the cases of delta_cases.py, host-fed.  Their GPU twins are in test_gpu_delta_snapshot.py."""

import pytest

from retina_amd import workloads as W

from . import delta_cases as D
from .growth_inputs import PARITY

BE = D.Backend(None)


@pytest.fixture(scope="module", autouse=True)
def lib():
    from retina_amd import _abi, build
    build.build()
    return _abi.load()


@pytest.mark.parametrize("name", PARITY)
def test_accumulation_across_specs(name):
    D.accumulation(BE, name)


def test_only_what_changed():
    D.only_what_changed(BE)


@pytest.mark.parametrize("name", ["local-all6", "c5-local"])
def test_idle(name):
    D.idle(BE, name)


def test_growth_between_deltas_wide():
    assert D.growth_between_deltas(BE, "small-wide", 4, sparse_capacity_log2=4, sparse_max_log2=20) == "cpu"


def test_growth_between_deltas_compact():
    D.growth_between_deltas(BE, "compact", 3, sparse_capacity_log2=8, sparse_max_log2=22)


@pytest.mark.parametrize("spec,remote", [(W.C1_REMOTE, True), (W.LOCAL_FWD_DROP, False)], ids=["wide", "dense"])
def test_retire(spec, remote):
    D.retire(BE, spec, remote)


def test_more_slots():
    D.more_slots(BE)


@pytest.mark.parametrize("spec,remote", [(W.C1_REMOTE, True), (W.LOCAL_FWD_DROP, False)], ids=["wide", "dense"])
def test_reset_and_reconcile(spec, remote):
    D.reset_and_reconcile(BE, spec, remote)


@pytest.mark.parametrize("name", ["local-c1-ip-ns-pod-wl", "remote-plain"])
def test_full_snapshots_between(name):
    D.full_snapshots_between(BE, name)


@pytest.mark.parametrize("kw", [{}, dict(sparse_capacity_log2=4, sparse_max_log2=20)], ids=["fixed", "growing"])
def test_import(kw):
    D.imported(BE, **kw)


def test_smallest_shapes():
    D.smallest_shapes(BE)
