"""Growth of the group-by table on the GPU (gpuagg_set_sparse_growth): a table that starts
far too small takes every key through the overflow list and the regrow kernels, for the
wide (192-bit keys) and the compact (64-bit DNS keys) layout, and the series equal the C
port exactly with nothing lost.  The CPU backend's cases are in test_sparse_growth_cpu.py."""

import numpy as np
import pytest

from retina_amd import _abi
from retina_amd import workloads as W

from .growth_inputs import (PARITY, WIDE_BYTES, canonical, dns_updates, ref_series, slices, snapshot_values,
                            wide_field_batch, wide_field_rows, workload)
from .helpers import diff_series, make_engine, to_device

pytestmark = pytest.mark.gpu


def _submit(g, recs, device, chunks=1, sync=True, pad=False):
    """Device-resident submits of `chunks` slices (a number, or their lengths), no sync
    between them.  Returns the device columns: the caller holds them until the launches
    that read them have been synced.  pad: every column is uploaded behind one more
    element and starts 4 bytes past a 16-byte boundary."""
    from retina_amd import GpuAgg
    keep = []
    for part in slices(recs, chunks):
        ts = to_device(part, device)
        if pad:
            import torch
            ts = [torch.cat([t.new_zeros(1), t])[1:] for t in ts]
            assert all(t.data_ptr() % 16 == 4 for t in ts)
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


# ---- growth x key layout x kernel --------------------------------------------------------
# Every run below starts at 2^4 slots and may reach 2^22, fed by three device submits with
# no sync between them, then a snapshot.

def _grown(device, name, flags=0, chunks=3, pad=False, **kw):
    """One engine run of input `name`: (series, table entries, facts about the run)."""
    pods, recs, spec, remote, _ = workload(name)
    kw.setdefault("sparse_max_log2", 22)
    g = make_engine(pods, spec, remote, device, recs, sparse_capacity_log2=4, flags=flags, **kw)
    try:
        cols = _submit(g, recs, device, chunks=chunks, sync=False, pad=pad)
        got = snapshot_values(g)
        del cols
        facts = dict(g.sparse_info(), regrow=g.regrow_kernel_name(), kernel=g.kernel_name(),
                     last_dropped=g.last_dropped, dropped=g.stats()["sparse_dropped"])
        return got, _entries(g, device).clone(), facts
    finally:
        g.close()


def _check_grown(name, got, facts, regrow="sparse_regrow_kernel"):
    want = workload(name)[4]
    assert got == want, diff_series(got, want)
    assert facts["last_dropped"] == 0 and facts["dropped"] == 0, facts
    assert facts["grows"] >= 1 and facts["overflow_replayed"] > 0, facts
    assert facts["regrow"] == regrow, facts


def _same_table(a, b):
    import torch
    (ka, va), (kb, vb) = _canonical(a), _canonical(b)
    assert ka.shape == kb.shape and torch.equal(ka, kb) and torch.equal(va, vb)


_DEFAULT = {}


def _default(device, name):
    """The default-flags run of `name`, once per process: what the flag runs compare with."""
    if (device, name) not in _DEFAULT:
        _DEFAULT[(device, name)] = _grown(device, name)
    return _DEFAULT[(device, name)]


def _vector_loads(kernel):
    """Whether the aggregation kernel named `kernel` is a 16-byte-load instantiation."""
    fn, args = kernel.rstrip(">").split("<", 1)
    args = [a.strip() for a in args.split(",")]
    at = {"aggregate_kernel": 0, "dense_local_kernel": 1, "dense_lds_kernel": 1}.get(fn)
    return True if at is None else args[at] == "true"  # (wide_kernel has no scalar form)


@pytest.mark.parametrize("name", PARITY)
def test_growth_by_key_layout(gpu_device, name):
    """Six specs of test_gpu_parity.CASES: wide keys with port fields and DNS ids through the
    overflow list, its replay and the regrow (the all6 ones), dense groups beside wide keys
    in the generic kernel (local-all6), compact keys (c5-local), edge rows.  The LDS regrow
    and the direct rehash build the same table."""
    got, ent, facts = _default(gpu_device, name)
    _check_grown(name, got, facts)
    if name == "local-all6":
        assert facts["kernel"] == "aggregate_kernel<true, false>"
    got_d, ent_d, facts_d = _grown(gpu_device, name, flags=_abi.FLAG_REGROW_DIRECT)
    _check_grown(name, got_d, facts_d, regrow="sparse_rehash_direct_kernel")
    _same_table(ent, ent_d)


FLAG_RUNS = [("no-hot-keys", _abi.FLAG_NO_HOT_KEYS), ("no-wide-lists", _abi.FLAG_NO_WIDE_LISTS),
             ("no-hot-keys-no-wide-lists", _abi.FLAG_NO_HOT_KEYS | _abi.FLAG_NO_WIDE_LISTS),
             ("fold-per-batch", _abi.FLAG_FOLD_PER_BATCH),
             # ignored by a plan with ports or DNS: a narrow entry has no room for them
             ("narrow-entries", _abi.FLAG_NARROW_ENTRIES)]


@pytest.mark.parametrize("flags", [f for _, f in FLAG_RUNS], ids=[i for i, _ in FLAG_RUNS])
@pytest.mark.parametrize("name", ["remote-all6-both", "local-all6"])
def test_growth_with_ports_and_dns_by_flag(gpu_device, name, flags):
    """The plans whose keys carry ports and DNS ids, under every flag that changes the way
    an update takes into the table: the same series and the same table, key for key, as the
    default run -- so no key lost a port or a DNS id on any of the ways."""
    got, ent, facts = _grown(gpu_device, name, flags=flags)
    _check_grown(name, got, facts)
    _same_table(ent, _default(gpu_device, name)[1])
    # the keys do carry them (a local-context key has no destination side)
    assert ((ent[:, 1] >> 47) & 0x1FFFF).ne(0).any() and (ent[:, 2] & 0xFFFFFFFF).ne(0).any()
    if name == "remote-all6-both":
        assert ((ent[:, 1] >> 30) & 0x1FFFF).ne(0).any()


def test_growth_with_sketches_on(gpu_device):
    """Count-min and HLL on: the series stay exact.  (The sketches run in a pass of their
    own -- the runtime clears the sketch arguments of the aggregation launch, so
    aggregate_kernel<., true> is not what runs here; this covers growth beside that pass.)"""
    got, ent, facts = _grown(gpu_device, "remote-plain", cms_depth=4, cms_width_log2=12, hll_precision=10)
    _check_grown("remote-plain", got, facts)
    _same_table(ent, _default(gpu_device, "remote-plain")[1])


@pytest.mark.parametrize("name", ["remote-all6-both", "local-all6", "c5-local"])
def test_growth_scalar_load_kernels(gpu_device, name):
    """Columns 4 bytes past a 16-byte boundary, slices of 9,999 / 10,002 / 9,999 records: the
    scalar-load instantiations produce the overflow entries."""
    got, ent, facts = _grown(gpu_device, name, chunks=[9_999, 10_002, 9_999], pad=True)
    assert not _vector_loads(facts["kernel"]), facts
    _check_grown(name, got, facts)
    _same_table(ent, _default(gpu_device, name)[1])


def test_growth_with_narrow_entries(gpu_device):
    """C1_REMOTE has neither ports nor DNS: here the 24-byte list entries are in use."""
    got, _, facts = _grown(gpu_device, "small-wide", flags=_abi.FLAG_NARROW_ENTRIES)
    _check_grown("small-wide", got, facts)


# ---- conservation while the list overflows -----------------------------------------------

def _fixed_table(device, name, lg):
    """The reference table of input `name`: canonical entries of an engine with a fixed
    2^lg-slot table whose series equal the C port's."""
    pods, recs, spec, remote, want = workload(name)
    g = make_engine(pods, spec, remote, device, recs, sparse_capacity_log2=lg)
    try:
        _submit(g, recs, device)
        got = snapshot_values(g)
        assert g.last_dropped == 0 and got == want, diff_series(got, want)
        return canonical(_entries(g, device).cpu().numpy())
    finally:
        g.close()


@pytest.fixture(scope="module")
def many_wide_fixed(gpu_device):
    return _fixed_table(gpu_device, "many-wide", 22)


def _lossy(device, name, **kw):
    """Three device submits without a sync into a table that cannot take them: (canonical
    table entries, lost updates), the loss read before and after a snapshot."""
    pods, recs, spec, remote, _ = workload(name)
    g = make_engine(pods, spec, remote, device, recs, **kw)
    try:
        cols = _submit(g, recs, device, chunks=3, sync=False)
        g.sync()
        del cols
        dropped = g.stats()["sparse_dropped"]
        ent = canonical(_entries(g, device).cpu().numpy())
        g.snapshot()
        assert dropped == g.last_dropped == g.stats()["sparse_dropped"]
        return ent, dropped
    finally:
        g.close()


def _check_partial(ent, ref):
    """Every exported key is one of the reference table's, with no more than its count and
    bytes (KeyError: a key the reference lacks)."""
    for key, (c, b) in ent.items():
        rc, rb = ref[key]
        assert 0 < c <= rc and b <= rb, (key, c, b, rc, rb)


def test_wide_conservation_while_list_overflows(gpu_device, many_wide_fixed):
    """4,096 slots, a 256-entry list and 329,728 keys in back-to-back submits: the first
    launch alone brings ~133k new keys, far more than table and list take before the table
    can grow.  What is lost is counted update for update (every record is one update), and
    what is kept is a part of the truth."""
    ent, dropped = _lossy(gpu_device, "many-wide", sparse_capacity_log2=12, sparse_max_log2=22,
                          sparse_overflow_entries=256)
    assert dropped > 0
    assert sum(c for c, _ in ent.values()) + dropped == 400_000
    _check_partial(ent, many_wide_fixed)


def test_wide_default_list_loses_nothing(many_wide_lds, many_wide_fixed):
    _, ent, _, lost = many_wide_lds
    assert lost == 0
    assert canonical(ent.cpu().numpy()) == many_wide_fixed


def test_compact_conservation_while_list_overflows(gpu_device):
    """The compact layout: the table may reach 2^10 slots only, the list holds 256 entries.
    The DNS updates of the C port (the sum of its request / response series) are in the
    table or counted as lost."""
    want = workload("compact")[4]
    ref = _fixed_table(gpu_device, "compact", 20)
    ent, dropped = _lossy(gpu_device, "compact", sparse_capacity_log2=8, sparse_max_log2=10,
                          sparse_overflow_entries=256)
    assert dropped > 0
    assert sum(c for c, _ in ent.values()) + dropped == dns_updates(want) == sum(c for c, _ in ref.values())
    _check_partial(ent, ref)


FEW_KEYS = dict(off={}, at_its_limit={"sparse_max_log2": 4},
                one_doubling={"sparse_max_log2": 5, "sparse_overflow_entries": 16})


@pytest.mark.parametrize("grow", list(FEW_KEYS))
def test_counted_entries_in_a_16_slot_table(gpu_device, grow):
    """Three keys, 18,000 records: every workgroup flushes its hot-key cache as entries of
    count > 1 into a one-segment table of 16 slots -- growth off, on with the table at its
    limit, and on with one doubling and a 16-entry list.  Nothing is lost."""
    pods, _ = wide_field_rows()
    recs = wide_field_batch(np.tile([0, 1, 2], 6_000), np.tile(WIDE_BYTES + (1,), 3_000))
    want = ref_series(pods, recs, W.C1_REMOTE, True)
    g = make_engine(pods, W.C1_REMOTE, True, gpu_device, sparse_capacity_log2=4, **FEW_KEYS[grow])
    try:
        cols = _submit(g, recs, gpu_device, chunks=2, sync=False)
        got = snapshot_values(g)
        del cols
        assert g.last_dropped == 0 and g.stats()["sparse_dropped"] == 0
        assert got == want, diff_series(got, want)
    finally:
        g.close()


def test_counted_entries_lost_at_a_full_table(gpu_device):
    """64 flows, 16 slots, growth off: the hot-key cache's entries of count > 1 find the
    table full, and each adds its whole count to the lost updates."""
    pods, _ = wide_field_rows()
    recs = W.gen_records(200_000, pods, seed=64, flows=64, flow_zipf=1.2, n_dst=64)
    g = make_engine(pods, W.C1_REMOTE, True, gpu_device, sparse_capacity_log2=4)
    try:
        cols = _submit(g, recs, gpu_device, chunks=2, sync=False)
        g.sync()
        del cols
        ent = _entries(g, gpu_device)
        dropped = g.stats()["sparse_dropped"]
        assert dropped > 0 and ent.shape[0] > 0
        assert int(ent[:, 3].sum().item()) + dropped == len(recs)
    finally:
        g.close()


# ---- the 2^24 boundary: above it a wide table is one segment without lists ------------------

@pytest.mark.parametrize("flags", [0, _abi.FLAG_NO_HOT_KEYS], ids=["default", "no-hot-keys"])
def test_fixed_table_above_the_wide_lists(gpu_device, flags):
    """2^25 slots: whole-table probing (kSparseMaxProbe) from the aggregation kernel, with
    and without the hot-key cache in front."""
    pods, recs, spec, remote, want = workload("small-wide")
    g = make_engine(pods, spec, remote, gpu_device, recs, sparse_capacity_log2=25, flags=flags)
    try:
        cols = _submit(g, recs, gpu_device, chunks=3, sync=False)
        got = snapshot_values(g)
        del cols
        assert g.kernel_name() == "aggregate_kernel<true, false>"  # (wide_kernel needs the lists)
        assert g.last_dropped == 0 and g.stats()["sparse_dropped"] == 0
        assert got == want, diff_series(got, want)
        assert g.sparse_info() == {"capacity_log2": 25, "grows": 0, "overflow_replayed": 0}
    finally:
        g.close()


def _synthetic_entries(lo, hi, device):
    """Entries lo .. hi - 1 of a table nobody aggregated: entry i has k0 = 1 << 63 | i, both
    port fields, the destination slot, the destination address and the DNS id non-zero
    functions of i (k2's top bit is clear, so it is never the all-ones pending mark),
    count i % 7 + 1 and 3 i + 1 bytes."""
    import torch
    i = torch.arange(lo, hi, dtype=torch.int64, device=device)
    e = torch.empty((hi - lo, 5), dtype=torch.int64, device=device)
    e[:, 0] = i | torch.iinfo(torch.int64).min
    e[:, 1] = _synthetic_k1(i)
    e[:, 2] = _synthetic_k2(i)
    e[:, 3] = i % 7 + 1
    e[:, 4] = 3 * i + 1
    return e


def _synthetic_k1(i):
    return (((i & 0x7FFF) + 1) << 47) | ((((i >> 3) & 0x7FFF) + 1) << 30) | ((i % 1000 + 1) << 9)


def _synthetic_k2(i):
    return (((i * 2654435761) & 0x7FFFFFFF) << 32) | (i % 65521 + 1)


def test_growth_across_the_wide_list_limit(gpu_device):
    """8.6M synthetic entries imported in two halves into a 2^23-slot table that may reach
    2^25.  The first half grows it to 2^24 with the LDS regrow at its largest (4,096
    segments); the second to 2^25, one segment, with the direct rehash.  Every key word and
    every count and byte sum comes out as it went in.  The load is at most ~52 % at every
    import, so probes stay short; past 100 % the whole-table probing of a table above 2^24
    would take billions of memory-side CAS.  Not covered for that reason: the replay of an
    overflow list into a table above 2^24."""
    import torch
    dev = torch.device("cuda", gpu_device)
    half, n = 4_300_000, 8_600_000
    pods, _, spec, remote, _ = workload("small-wide")
    g = make_engine(pods, spec, remote, gpu_device, sparse_capacity_log2=23, sparse_max_log2=25)
    try:
        for lo, lg, kernel in ((0, 24, "sparse_regrow_kernel"), (half, 25, "sparse_rehash_direct_kernel")):
            e = _synthetic_entries(lo, lo + half, dev)
            g.sparse_import(e.data_ptr(), e.shape[0])
            g.sync()
            assert g.sparse_info()["capacity_log2"] == lg and g.regrow_kernel_name() == kernel
            del e
        out = torch.empty((1 << 24, 5), dtype=torch.int64, device=dev)
        m = g.sparse_export(out.data_ptr(), out.shape[0])
        out = out[:m]
        assert g.stats()["sparse_dropped"] == 0
    finally:
        g.close()
    i = out[:, 0] & 0xFFFFFFFF
    assert int(i.max()) < n
    assert torch.equal(out[:, 0], i | torch.iinfo(torch.int64).min)
    assert torch.equal(out[:, 1], _synthetic_k1(i)) and torch.equal(out[:, 2], _synthetic_k2(i))
    sums = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    sums.index_add_(0, i, out[:, 3:5])
    every = torch.arange(n, dtype=torch.int64, device=dev)
    assert torch.equal(sums[:, 0], every % 7 + 1) and torch.equal(sums[:, 1], 3 * every + 1)


def test_import_in_steps_of_the_list(gpu_device):
    """17,421 entries into a 16-slot table with a 256-entry list: gpuagg_sparse_import takes
    them in 69 steps of the list's size, settling after each, and loses nothing."""
    pods, recs, spec, remote, want = workload("small-wide")
    a = make_engine(pods, spec, remote, gpu_device, recs, sparse_capacity_log2=20)
    b = make_engine(pods, spec, remote, gpu_device, recs, sparse_capacity_log2=4, sparse_max_log2=20,
                    sparse_overflow_entries=256)
    try:
        _submit(a, recs, gpu_device)
        ent = _entries(a, gpu_device)
        assert -(-ent.shape[0] // 256) == 69
        b.sparse_import(ent.data_ptr(), ent.shape[0])
        got = snapshot_values(b)
        assert b.last_dropped == 0 and b.stats()["sparse_dropped"] == 0
        assert got == want, diff_series(got, want)
        assert b.sparse_info()["grows"] >= 1
    finally:
        a.close()
        b.close()


# ---- after a grow ------------------------------------------------------------------------

def test_reconcile_layouts_on_a_grown_table(gpu_device):
    """A wide table grown from 16 slots, then the compact plan on it (reconcile), then the
    wide plan again: each plan's records give the C port's series."""
    pods, recs_w, spec_w, remote, want_w = workload("local-c1-ip-ns-pod-wl")
    _, recs_c, spec_c, _, want_c = workload("c5-local")
    g = make_engine(pods, spec_w, remote, gpu_device, recs_c, sparse_capacity_log2=4, sparse_max_log2=22)
    try:
        for spec, recs, want in ((spec_w, recs_w, want_w), (spec_c, recs_c, want_c), (spec_w, recs_w, want_w)):
            g.reconcile(spec)
            cols = _submit(g, recs, gpu_device, chunks=3, sync=False)
            got = snapshot_values(g)
            del cols
            assert g.last_dropped == 0
            assert got == want, diff_series(got, want)
            assert g.sparse_info()["grows"] >= 1
    finally:
        g.close()


def test_reset_after_a_grow(gpu_device):
    """gpuagg_reset empties the grown table and keeps its size: the same records again fit
    without another trip through the overflow list."""
    pods, recs, spec, remote, want = workload("local-c1-ip-ns-pod-wl")
    g = make_engine(pods, spec, remote, gpu_device, recs, sparse_capacity_log2=4, sparse_max_log2=22)
    try:
        cols = _submit(g, recs, gpu_device, chunks=3, sync=False)
        assert snapshot_values(g) == want
        info = g.sparse_info()
        assert info["grows"] >= 1 and info["overflow_replayed"] > 0
        g.reset()
        assert g.snapshot() == {}
        assert g.sparse_info()["capacity_log2"] == info["capacity_log2"]
        cols = _submit(g, recs, gpu_device, chunks=3, sync=False)
        got = snapshot_values(g)
        del cols
        assert g.last_dropped == 0 and g.stats()["sparse_dropped"] == 0
        assert got == want, diff_series(got, want)
        assert g.sparse_info()["overflow_replayed"] == info["overflow_replayed"]
    finally:
        g.close()
