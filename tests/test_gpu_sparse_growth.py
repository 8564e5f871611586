"""Growth of the group-by table on the GPU (gpuagg_set_sparse_growth): a table that starts
far too small takes every key through the overflow list and the regrow kernels, for the
wide (192-bit keys) and the compact (64-bit DNS keys) layout, and the series equal the C
port exactly with nothing lost.  The CPU backend's cases are in test_sparse_growth_cpu.py."""

import pytest

from .growth_inputs import slices, snapshot_values, workload
from .helpers import diff_series, make_engine, to_device

pytestmark = pytest.mark.gpu


def _submit(g, recs, device, chunks=1, sync=True):
    """Device-resident submits of `chunks` slices, no sync between them.  Returns the device
    columns: the caller holds them until the launches that read them have been synced."""
    from retina_amd import GpuAgg
    keep = []
    for part in slices(recs, chunks):
        ts = to_device(part, device)
        keep.append(ts)
        g.submit_device(GpuAgg.device_columns(*ts), len(part))
    if sync:
        g.sync()
    return keep


def _entries(g, device):
    """The exported table: (n, 5) int64 entries on the device."""
    import torch
    cap = int(g.state().sparse_len)
    out = torch.empty((cap, 5), dtype=torch.int64, device=torch.device("cuda", device))
    n = g.sparse_export(out.data_ptr(), cap)
    return out[:n]


def _canonical(e):
    """(k0, k1, k2) -> (count, bytes) tensors, sorted by key, duplicate slots summed."""
    import torch
    keys, inv = torch.unique(e[:, :3], dim=0, return_inverse=True)
    vals = torch.zeros((keys.shape[0], 2), dtype=torch.int64, device=e.device)
    vals.index_add_(0, inv, e[:, 3:5])
    return keys, vals


def test_wide_below_one_segment_into_several(gpu_device):
    """The input of test_full_table_reports_loss: 16 slots, 17,421 keys.  The table crosses
    every segment size from 2^4 to 2^12 and the step from one segment to several."""
    pods, recs, spec, remote, want = workload("small-wide")
    g = make_engine(pods, spec, remote, gpu_device, recs, sparse_capacity_log2=4, sparse_max_log2=20)
    try:
        _submit(g, recs, gpu_device)
        got = snapshot_values(g)
        info = g.sparse_info()
        assert g.last_dropped == 0 and g.stats()["sparse_dropped"] == 0
        assert got == want, diff_series(got, want)
        assert info["capacity_log2"] == 16 and info["grows"] >= 1 and info["overflow_replayed"] > 0, info
    finally:
        g.close()


def _many_wide(device, flags, series=True):
    """329,728 distinct keys into a table of one full segment (2^12), three submits without
    a sync between them; returns (series, table entries, sparse_info, lost updates)."""
    pods, recs, spec, remote, _ = workload("many-wide")
    g = make_engine(pods, spec, remote, device, recs, sparse_capacity_log2=12, sparse_max_log2=22, flags=flags)
    try:
        cols = _submit(g, recs, device, chunks=3, sync=False)
        got = snapshot_values(g) if series else None
        g.sync()
        del cols
        info = dict(g.sparse_info(), kernel=g.regrow_kernel_name())
        return got, _entries(g, device).clone(), info, g.stats()["sparse_dropped"]
    finally:
        g.close()


@pytest.fixture(scope="module")
def many_wide_lds(gpu_device):
    return _many_wide(gpu_device, 0)


def test_wide_multi_doubling_from_one_segment(gpu_device, many_wide_lds):
    import torch
    want = workload("many-wide")[4]
    got, ent, info, lost = many_wide_lds
    assert lost == 0
    assert got == want, diff_series(got, want)
    assert info["capacity_log2"] == 20 and info["grows"] >= 1, info
    # the regrow merges the duplicate slots a wide table may hold, and the list's replay
    # waits for a key being published: one slot per key
    assert torch.unique(ent[:, :3], dim=0).shape[0] == ent.shape[0] == len(want) // 2


def test_lds_regrow_equals_direct_rehash(gpu_device, many_wide_lds):
    import torch
    from retina_amd import _abi
    got, ent, info, lost = many_wide_lds
    _, ent_d, info_d, lost_d = _many_wide(gpu_device, _abi.FLAG_REGROW_DIRECT, series=False)
    assert lost == 0 and lost_d == 0
    assert info_d["capacity_log2"] == info["capacity_log2"]
    assert info["kernel"] == "sparse_regrow_kernel" and info_d["kernel"] == "sparse_rehash_direct_kernel"
    (ka, va), (kb, vb) = _canonical(ent), _canonical(ent_d)
    assert torch.equal(ka, kb) and torch.equal(va, vb)


def test_compact_layout(gpu_device):
    pods, recs, spec, remote, want = workload("compact")
    g = make_engine(pods, spec, remote, gpu_device, recs, sparse_capacity_log2=8, sparse_max_log2=22)
    try:
        cols = _submit(g, recs, gpu_device, chunks=3, sync=False)
        got = snapshot_values(g)
        del cols
        info = g.sparse_info()
        assert g.regrow_kernel_name() == "sparse_regrow_kernel"
        assert info["capacity_log2"] > 8 and info["grows"] >= 1, info  # the input does outgrow 2^8
        assert g.last_dropped == 0 and g.stats()["sparse_dropped"] == 0
        assert got == want, diff_series(got, want)
    finally:
        g.close()


def test_growth_on_import(gpu_device):
    """A fixed 2^20 table's entries imported into a 16-slot table with growth on."""
    pods, recs, spec, remote, want = workload("small-wide")
    a = make_engine(pods, spec, remote, gpu_device, recs, sparse_capacity_log2=20)
    b = make_engine(pods, spec, remote, gpu_device, recs, sparse_capacity_log2=4, sparse_max_log2=20)
    try:
        _submit(a, recs, gpu_device)
        ent = _entries(a, gpu_device)
        b.sparse_import(ent.data_ptr(), ent.shape[0])
        got_a, got_b = snapshot_values(a), snapshot_values(b)
        assert b.last_dropped == 0 and b.stats()["sparse_dropped"] == 0
        assert got_b == got_a == want, diff_series(got_b, want)
        assert b.sparse_info()["capacity_log2"] == 16
    finally:
        a.close()
        b.close()


def test_merge_with_pending_overflow(gpu_device):
    """gpuagg_merge (peer copies, one device) of three contexts that start at 16 slots and
    were never synced: their lists are not empty when the merge starts, and each grows
    inside it, before its export buffer is sized."""
    from retina_amd import dist as D
    pods, recs, spec, remote, want = workload("small-wide")
    parts = [make_engine(pods, spec, remote, gpu_device, recs, sparse_capacity_log2=4, sparse_max_log2=20)
             for _ in range(3)]
    try:
        cols = [_submit(g, D.shard_records(recs, 3, r), gpu_device, sync=False) for r, g in enumerate(parts)]
        parts[0].merge_from(parts[1:])
        got = snapshot_values(parts[0])
        del cols
        assert parts[0].last_dropped == 0
        assert got == want, diff_series(got, want)
        assert [p.snapshot() for p in parts[1:]] == [{}, {}]
        assert all(p.sparse_info()["grows"] >= 1 for p in parts)
        assert parts[0].sparse_info()["capacity_log2"] == 16
    finally:
        for p in parts:
            p.close()


def test_retire_with_pending_overflow(gpu_device):
    """gpuagg_retire_slots exports the table of a context that was never synced."""
    from retina_amd import workloads as W
    pods, recs, spec, remote, want = workload("small-wide")
    g = make_engine(pods, spec, remote, gpu_device, recs, sparse_capacity_log2=4, sparse_max_log2=20,
                    max_ips=len(pods.ips) + 16)
    try:
        g.cache_update_endpoint(W.Endpoint("ghost", "ghost-0", [0xFEFEFEFE], None))  # a pod no record names
        g.cache_commit(1)
        cols = _submit(g, recs, gpu_device, sync=False)
        g.cache_delete_endpoint("ghost", "ghost-0")
        g.cache_commit(2)
        assert g.retire_slots() == 1
        got = snapshot_values(g)
        del cols
        assert g.last_dropped == 0 and g.sparse_info()["capacity_log2"] == 16
        assert got == want, diff_series(got, want)
    finally:
        g.close()


def test_residual_loss_is_counted(gpu_device):
    """The table may reach 2^8 slots only and the list holds 256 entries: what does not fit
    is counted, update for update (every C1_REMOTE record is one forward or drop update)."""
    pods, recs, spec, remote, _ = workload("small-wide")
    g = make_engine(pods, spec, remote, gpu_device, recs, sparse_capacity_log2=4, sparse_max_log2=8,
                    sparse_overflow_entries=256)
    try:
        _submit(g, recs, gpu_device)
        g.snapshot()
        assert g.last_dropped > 0
        ent = _entries(g, gpu_device)
        dropped = g.stats()["sparse_dropped"]
        assert dropped == g.last_dropped
        assert int(ent[:, 3].sum().item()) + dropped == len(recs) == 20_000
        assert g.sparse_info()["capacity_log2"] == 8
    finally:
        g.close()


def test_off_means_off(gpu_device):
    """No setter call: the 16-slot table of test_full_table_reports_loss stays and loses."""
    pods, recs, spec, remote, _ = workload("small-wide")
    g = make_engine(pods, spec, remote, gpu_device, sparse_capacity_log2=4)
    try:
        _submit(g, recs, gpu_device)
        got = g.snapshot()
        assert g.sparse_info() == {"capacity_log2": 4, "grows": 0, "overflow_replayed": 0}
        assert g.last_dropped > 0 and len(got) > 0
    finally:
        g.close()
