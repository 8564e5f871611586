"""Growth of the group-by table on the CPU backend (gpuagg_set_sparse_growth,
GPUAGG_FLAG_CPU_BACKEND): a table that starts far too small takes every key through the
overflow list and the regrow, and the series equal the C port exactly.  The GPU cases are
in test_gpu_sparse_growth.py."""

import functools

import numpy as np
import pytest

from .growth_inputs import PARITY, canonical, dns_updates, slices, snapshot_values, workload
from .helpers import diff_series, make_engine

CPU = 128  # GPUAGG_FLAG_CPU_BACKEND


@pytest.fixture(scope="module", autouse=True)
def lib():
    from retina_amd import _abi, build
    build.build()
    return _abi.load()


def _export(g):
    cap = int(g.state().sparse_len)
    out = np.zeros((cap, 5), np.uint64)
    n = g.sparse_export(out.ctypes.data, cap)
    return out[:n]


def test_wide_below_one_segment_into_several():
    """16 slots, 17,421 keys: the table crosses every segment size from 2^4 to 2^12 and the
    step from one segment to several, nothing is lost."""
    pods, recs, spec, remote, want = workload("small-wide")
    g = make_engine(pods, spec, remote, recs=recs, flags=CPU, sparse_capacity_log2=4, sparse_max_log2=20)
    try:
        g.submit_numpy(recs)
        got = snapshot_values(g)
        info = g.sparse_info()
        assert g.last_dropped == 0 and g.stats()["sparse_dropped"] == 0
        assert got == want, diff_series(got, want)
        assert info["capacity_log2"] == 16 and info["grows"] >= 1 and info["overflow_replayed"] > 0, info
    finally:
        g.close()


def test_compact_layout():
    pods, recs, spec, remote, want = workload("compact")
    g = make_engine(pods, spec, remote, recs=recs, flags=CPU, sparse_capacity_log2=8, sparse_max_log2=22)
    try:
        for part in slices(recs, 3):
            g.submit_numpy(part)
        got = snapshot_values(g)
        info = g.sparse_info()
        assert info["capacity_log2"] > 8 and info["grows"] >= 1, info
        assert g.last_dropped == 0
        assert got == want, diff_series(got, want)
    finally:
        g.close()


def test_growth_on_import():
    """A fixed 2^20 table's entries imported into a 16-slot table with growth on."""
    pods, recs, spec, remote, want = workload("small-wide")
    a = make_engine(pods, spec, remote, recs=recs, flags=CPU, sparse_capacity_log2=20)
    b = make_engine(pods, spec, remote, recs=recs, flags=CPU, sparse_capacity_log2=4, sparse_max_log2=20)
    try:
        a.submit_numpy(recs)
        ent = _export(a)
        assert a.sparse_info() == {"capacity_log2": 20, "grows": 0, "overflow_replayed": 0}
        b.sparse_import(ent.ctypes.data, len(ent))
        got_a, got_b = snapshot_values(a), snapshot_values(b)
        assert b.last_dropped == 0 and b.stats()["sparse_dropped"] == 0
        assert got_b == got_a == want, diff_series(got_b, want)
        assert b.sparse_info()["capacity_log2"] == 16
    finally:
        a.close()
        b.close()


def test_residual_loss_is_counted():
    """The table may reach 2^8 slots only and the list holds 256 entries: what does not fit
    is counted, update for update."""
    pods, recs, spec, remote, _ = workload("small-wide")
    g = make_engine(pods, spec, remote, recs=recs, flags=CPU, sparse_capacity_log2=4, sparse_max_log2=8,
                    sparse_overflow_entries=256)
    try:
        g.submit_numpy(recs)
        g.snapshot()
        assert g.last_dropped > 0
        ent = _export(g)
        dropped = g.stats()["sparse_dropped"]
        assert dropped == g.last_dropped
        assert int(ent[:, 3].sum()) + dropped == len(recs) == 20_000
        assert len(canonical(ent)) == len(ent)  # the CPU table holds a key once
        assert g.sparse_info()["capacity_log2"] == 8
    finally:
        g.close()


def test_merge_with_pending_overflow():
    """gpuagg_merge of three contexts that start at 16 slots and were never synced: each
    settles (and grows) inside the merge, before its export buffer is sized."""
    from retina_amd import dist as D
    pods, recs, spec, remote, want = workload("small-wide")
    parts = [make_engine(pods, spec, remote, recs=recs, flags=CPU, sparse_capacity_log2=4, sparse_max_log2=20)
             for _ in range(3)]
    try:
        for r, g in enumerate(parts):
            g.submit_numpy(D.shard_records(recs, 3, r))
        parts[0].merge_from(parts[1:])
        got = snapshot_values(parts[0])
        assert parts[0].last_dropped == 0
        assert got == want, diff_series(got, want)
        assert [p.snapshot() for p in parts[1:]] == [{}, {}]
        assert all(p.sparse_info()["grows"] >= 1 and p.regrow_kernel_name() == "cpu" for p in parts)
        assert parts[0].sparse_info()["capacity_log2"] == 16
    finally:
        for p in parts:
            p.close()


def test_retire_with_pending_overflow():
    """gpuagg_retire_slots exports the table of a context that was never synced."""
    from retina_amd import workloads as W
    pods, recs, spec, remote, want = workload("small-wide")
    g = make_engine(pods, spec, remote, recs=recs, flags=CPU, sparse_capacity_log2=4, sparse_max_log2=20,
                    max_ips=len(pods.ips) + 16)
    try:
        g.cache_update_endpoint(W.Endpoint("ghost", "ghost-0", [0xFEFEFEFE], None))  # a pod no record names
        g.cache_commit(1)
        g.submit_numpy(recs)
        g.cache_delete_endpoint("ghost", "ghost-0")
        g.cache_commit(2)
        assert g.retire_slots() == 1
        got = snapshot_values(g)
        assert g.last_dropped == 0 and g.sparse_info()["capacity_log2"] == 16
        assert got == want, diff_series(got, want)
    finally:
        g.close()


def test_setter_arguments():
    from retina_amd.engine import GpuAggError
    pods, recs, spec, remote, _ = workload("small-wide")
    for bad in (3, 31):  # below the table's size, beyond 2^30
        with pytest.raises(GpuAggError):
            make_engine(pods, spec, remote, flags=CPU, sparse_capacity_log2=4, sparse_max_log2=bad)
    g = make_engine(pods, spec, remote, flags=CPU, sparse_capacity_log2=4)
    try:
        assert g.sparse_info() == {"capacity_log2": 4, "grows": 0, "overflow_replayed": 0}
    finally:
        g.close()


# ---- growth x key layout: the twins of test_gpu_sparse_growth.py, host-fed ----------------

@pytest.mark.parametrize("name", PARITY)
def test_growth_by_key_layout(name):
    """Six specs of test_gpu_parity.CASES from a 16-slot table, three host-fed slices: wide
    keys with port fields and DNS ids, dense groups beside wide keys, compact keys, edge
    rows."""
    pods, recs, spec, remote, want = workload(name)
    g = make_engine(pods, spec, remote, recs=recs, flags=CPU, sparse_capacity_log2=4, sparse_max_log2=22)
    try:
        for part in slices(recs, 3):
            g.submit_numpy(part)
        got = snapshot_values(g)
        info = g.sparse_info()
        assert g.last_dropped == 0 and g.stats()["sparse_dropped"] == 0
        assert got == want, diff_series(got, want)
        assert info["grows"] >= 1 and info["overflow_replayed"] > 0, info
        assert g.regrow_kernel_name() == "cpu"
    finally:
        g.close()


# ---- conservation while the list overflows -------------------------------------------------
# (the CPU backend grows the table at a sync only, not between submits: it loses far more
# than the GPU does on the same input -- what is asserted is that every update is either in
# the table or counted, not how many)

@functools.lru_cache(maxsize=None)
def _fixed_table(name, lg):
    """The reference table of an input, once per process: canonical entries of an engine
    with a fixed 2^lg-slot table whose series equal the C port's."""
    pods, recs, spec, remote, want = workload(name)
    g = make_engine(pods, spec, remote, recs=recs, flags=CPU, sparse_capacity_log2=lg)
    try:
        g.submit_numpy(recs)
        got = snapshot_values(g)
        assert g.last_dropped == 0 and got == want, diff_series(got, want)
        return canonical(_export(g))
    finally:
        g.close()


def _lossy(name, **kw):
    pods, recs, spec, remote, _ = workload(name)
    g = make_engine(pods, spec, remote, recs=recs, flags=CPU, **kw)
    try:
        for part in slices(recs, 3):
            g.submit_numpy(part)
        g.sync()
        dropped = g.stats()["sparse_dropped"]
        ent = canonical(_export(g))
        g.snapshot()
        assert dropped == g.last_dropped == g.stats()["sparse_dropped"]
        return ent, dropped
    finally:
        g.close()


def _check_partial(ent, ref):
    for key, (c, b) in ent.items():
        rc, rb = ref[key]  # (KeyError: a key the reference table lacks)
        assert 0 < c <= rc and b <= rb, (key, c, b, rc, rb)


@pytest.mark.parametrize("entries", [256, 0], ids=["256-entry-list", "default-list"])
def test_wide_conservation_while_list_overflows(entries):
    ref = _fixed_table("many-wide", 22)
    ent, dropped = _lossy("many-wide", sparse_capacity_log2=12, sparse_max_log2=22, sparse_overflow_entries=entries)
    assert sum(c for c, _ in ent.values()) + dropped == 400_000
    _check_partial(ent, ref)
    if entries:
        assert dropped > 0
    else:
        assert dropped == 0 and ent == ref


def test_compact_conservation_while_list_overflows():
    want = workload("compact")[4]
    ref = _fixed_table("compact", 20)
    ent, dropped = _lossy("compact", sparse_capacity_log2=8, sparse_max_log2=10, sparse_overflow_entries=256)
    assert dropped > 0
    assert sum(c for c, _ in ent.values()) + dropped == dns_updates(want) == sum(c for c, _ in ref.values())
    _check_partial(ent, ref)


def test_import_in_steps_of_the_list():
    """17,421 entries into a 16-slot table with a 256-entry list: 69 steps, nothing lost."""
    pods, recs, spec, remote, want = workload("small-wide")
    a = make_engine(pods, spec, remote, recs=recs, flags=CPU, sparse_capacity_log2=20)
    b = make_engine(pods, spec, remote, recs=recs, flags=CPU, sparse_capacity_log2=4, sparse_max_log2=20,
                    sparse_overflow_entries=256)
    try:
        a.submit_numpy(recs)
        ent = _export(a)
        assert -(-len(ent) // 256) == 69
        b.sparse_import(ent.ctypes.data, len(ent))
        got = snapshot_values(b)
        assert b.last_dropped == 0 and b.stats()["sparse_dropped"] == 0
        assert got == want, diff_series(got, want)
        assert b.sparse_info()["grows"] >= 1
    finally:
        a.close()
        b.close()


# ---- after a grow ------------------------------------------------------------------------

def test_reconcile_layouts_on_a_grown_table():
    """A wide table grown from 16 slots, then the compact plan on it, then the wide plan
    again: each plan's records give the C port's series."""
    pods, recs_w, spec_w, remote, want_w = workload("local-c1-ip-ns-pod-wl")
    _, recs_c, spec_c, _, want_c = workload("c5-local")
    g = make_engine(pods, spec_w, remote, recs=recs_c, flags=CPU, sparse_capacity_log2=4, sparse_max_log2=22)
    try:
        for spec, recs, want in ((spec_w, recs_w, want_w), (spec_c, recs_c, want_c), (spec_w, recs_w, want_w)):
            g.reconcile(spec)
            for part in slices(recs, 3):
                g.submit_numpy(part)
            got = snapshot_values(g)
            assert g.last_dropped == 0
            assert got == want, diff_series(got, want)
            assert g.sparse_info()["grows"] >= 1
    finally:
        g.close()


def test_reset_after_a_grow():
    """gpuagg_reset empties the grown table and keeps its size: the same records again fit
    without another trip through the overflow list."""
    pods, recs, spec, remote, want = workload("local-c1-ip-ns-pod-wl")
    g = make_engine(pods, spec, remote, recs=recs, flags=CPU, sparse_capacity_log2=4, sparse_max_log2=22)
    try:
        g.submit_numpy(recs)
        assert snapshot_values(g) == want
        info = g.sparse_info()
        assert info["grows"] >= 1 and info["overflow_replayed"] > 0
        g.reset()
        assert g.snapshot() == {}
        assert g.sparse_info()["capacity_log2"] == info["capacity_log2"]
        g.submit_numpy(recs)
        got = snapshot_values(g)
        assert g.last_dropped == 0 and g.stats()["sparse_dropped"] == 0
        assert got == want, diff_series(got, want)
        assert g.sparse_info()["overflow_replayed"] == info["overflow_replayed"]
    finally:
        g.close()
