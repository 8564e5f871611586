"""The delta-snapshot cases (gpuagg_snapshot_delta), written once and run on both backends:
test_delta_snapshot_cpu.py (GPUAGG_FLAG_CPU_BACKEND, host-fed) and
test_gpu_delta_snapshot.py (gfx950, device-resident submits).

What defines correctness everywhere: `acc`, the per-series sum (mod 2^64) of the deltas
since the last rebased one, equals gpuagg_snapshot at the same point for every series the
snapshot returns."""

from __future__ import annotations

import numpy as np

from oracle.ref_cpu import values_only
from retina_amd import workloads as W

from .growth_inputs import canonical, ref_series, slices, take, workload
from .helpers import diff_series, make_engine, to_device

CPU = 128  # GPUAGG_FLAG_CPU_BACKEND
M64 = (1 << 64) - 1


class Backend:
    """device None: the CPU backend, host-fed; else that GPU, device-resident submits."""

    def __init__(self, device=None):
        self.device = device

    def engine(self, pods, spec, remote, recs=None, flags=0, **kw):
        if self.device is None:
            return make_engine(pods, spec, remote, recs=recs, flags=CPU | flags, **kw)
        return make_engine(pods, spec, remote, self.device, recs, flags=flags, **kw)

    def submit(self, g, recs):
        if self.device is None:
            g.submit_numpy(recs)
            return
        from retina_amd import GpuAgg
        cols = to_device(recs, self.device)
        g.submit_device(GpuAgg.device_columns(*cols), len(recs))
        g.sync()  # (the columns are read until here)

    def entries(self, g) -> np.ndarray:
        """The exported table: (n, 5) uint64 entries on the host."""
        cap = int(g.state().sparse_len)
        if self.device is None:
            out = np.zeros((cap, 5), np.uint64)
            n = g.sparse_export(out.ctypes.data, cap)
            return out[:n]
        import torch
        out = torch.empty((cap, 5), dtype=torch.int64, device=torch.device("cuda", self.device))
        n = g.sparse_export(out.data_ptr(), cap)
        return out[:n].cpu().numpy().view(np.uint64)

    def import_entries(self, g, ent: np.ndarray):
        ent = np.ascontiguousarray(ent)
        if self.device is None:
            g.sparse_import(ent.ctypes.data, len(ent))
            return
        import torch
        t = torch.from_numpy(ent.view(np.int64)).to(torch.device("cuda", self.device))
        g.sparse_import(t.data_ptr(), len(ent))


class Acc:
    """The consumer of an engine's deltas: replaces on a rebased one, else adds."""

    def __init__(self, g):
        self.g, self.acc, self.rebased, self.deltas = g, {}, [], []

    def step(self):
        d, reb = self.g.snapshot_delta()
        if reb:
            self.acc = {}
        for k, v in d.items():
            self.acc[k] = (self.acc.get(k, 0) + v) & M64
        self.rebased.append(reb)
        self.deltas.append(d)
        return d, reb

    def check(self):
        """acc == gpuagg_snapshot, series for series."""
        snap = self.g.snapshot()
        assert self.acc == snap, diff_series(self.acc, snap)
        return snap

    def check_on_snapshot(self):
        """acc equals the snapshot on every series the snapshot returns."""
        snap = self.g.snapshot()
        sub = {k: self.acc.get(k) for k in snap}
        assert sub == snap, diff_series(sub, snap)
        return snap


# ---- 1 ------------------------------------------------------------------------------------
def accumulation(be: Backend, name: str):
    pods, recs, spec, remote, want = workload(name)
    g = be.engine(pods, spec, remote, recs)
    try:
        a = Acc(g)
        for part in slices(recs, 3):
            be.submit(g, part)
            a.step()
            a.check()
        assert a.rebased == [True, False, False]
        got = values_only(a.acc)
        assert got == want, diff_series(got, want)
        assert g.last_dropped == 0
    finally:
        g.close()


# ---- 2 ------------------------------------------------------------------------------------
def only_what_changed(be: Backend):
    pods, recs, spec, remote, _ = workload("many-wide")
    few = take(recs, slice(0, 1000))
    want = {k: v for k, v in ref_series(pods, few, spec, remote).items() if v}
    g = be.engine(pods, spec, remote, recs)
    try:
        be.submit(g, recs)
        n1, reb1 = g.snapshot_delta_count()  # (1.3M series: counted, not walked)
        before = canonical(be.entries(g))
        assert reb1 and n1 > 0
        be.submit(g, few)
        d, reb2 = g.snapshot_delta()
        info = g.delta_info()
        ent = be.entries(g)
        after = canonical(ent)
        assert not reb2
        got = values_only({k: v for k, v in d.items() if v})
        assert got == want, diff_series(got, want)
        assert set(values_only(d)) <= set(ref_series(pods, few, spec, remote))
        assert info["slots_scanned"] == int(g.state().sparse_len) == 1 << g.sparse_info()["capacity_log2"]
        changed = sum(1 for k, v in after.items() if before.get(k) != v)
        assert 0 < changed <= 1000
        assert changed <= info["changed_entries"] <= changed + (len(ent) - len(after)), (info, changed)
        assert info["changed_bins"] == 0 and info["rebases"] == 1
    finally:
        g.close()


# ---- 3 ------------------------------------------------------------------------------------
def idle(be: Backend, name: str):
    pods, recs, spec, remote, _ = workload(name)
    g = be.engine(pods, spec, remote, recs)
    try:
        be.submit(g, recs)
        d1, reb1 = g.snapshot_delta()
        d2, reb2 = g.snapshot_delta()
        info = g.delta_info()
        assert reb1 and d1 == g.snapshot() and len(d1) > 0
        assert d2 == {} and not reb2
        assert info["changed_entries"] == 0 and info["changed_bins"] == 0 and info["rebases"] == 1, info
    finally:
        g.close()


# ---- 4 ------------------------------------------------------------------------------------
def growth_between_deltas(be: Backend, name: str, chunks: int, flags: int = 0, **kw):
    pods, recs, spec, remote, want = workload(name)
    g = be.engine(pods, spec, remote, recs, flags=flags, **kw)
    try:
        a = Acc(g)
        grows = []
        for part in slices(recs, chunks):
            be.submit(g, part)
            a.step()
            grows.append(g.sparse_info()["grows"])
            a.check()
            assert g.last_dropped == 0
        assert a.rebased == [True] + [False] * (chunks - 1)
        assert any(y > x for x, y in zip(grows[:-1], grows[1:])), grows  # the table grew between two deltas
        got = values_only(a.acc)
        assert got == want, diff_series(got, want)
        return g.regrow_kernel_name()
    finally:
        g.close()


# ---- 5 ------------------------------------------------------------------------------------
def _without(recs, ips):
    """The rows of recs that name none of `ips`."""
    bad = np.isin(recs.src_ip, ips) | np.isin(recs.dst_ip, ips)
    return take(recs, np.flatnonzero(~bad))


def retire(be: Backend, spec, remote: bool):
    """A third of the pods leave.  Group-by entries move (the table is rebuilt without the
    dead pods' entries), dense bins are zeroed in the state and the baseline alike."""
    pods = W.make_pods(300, seed=21, apiserver=False)
    recs = W.gen_records(40_000, pods, seed=22, pod_frac=0.9)
    gone = [e for i, e in enumerate(pods.endpoints) if i % 3 == 1]
    gone_ips = np.array([ip for e in gone for ip in e.ips], np.uint32)
    gone_names = {e.name for e in gone}
    g = be.engine(pods, spec, remote, recs, max_ips=len(pods.ips) + 64, sparse_capacity_log2=16)
    try:
        a = Acc(g)
        be.submit(g, recs)
        a.step()
        first = a.check()
        for e in gone:
            g.cache_delete_endpoint(e.namespace, e.name)
        g.cache_commit(2)
        assert g.retire_slots() == len(gone)
        rest = _without(W.gen_records(40_000, pods, seed=23, pod_frac=0.9), gone_ips)
        assert 5_000 < len(rest) < 40_000
        be.submit(g, rest)
        _, reb = a.step()
        assert not reb
        snap = a.check_on_snapshot()

        def of_gone(k):
            return any(n.endswith("podname") and v in gone_names for n, v in k[1])
        retired = {k for k in first if of_gone(k)}
        assert len(retired) > 100 and len(snap) > 100
        assert not any(of_gone(k) for k in snap)
        assert all(a.acc[k] == first[k] for k in retired)  # their last accumulated value
        # a new pod takes a freed slot: it starts from zero in the state and in the baseline
        new_ip = W.ip_le(10, 250, 0, 1)
        g.cache_update_endpoint(W.Endpoint("ns-new", "pod-new", [new_ip], None))
        g.cache_commit(3)
        mine = take(rest, slice(0, 2_000))
        mine.src_ip[:] = new_ip
        be.submit(g, mine)
        _, reb = a.step()
        assert not reb
        snap = a.check_on_snapshot()
        assert any(("source_podname", "pod-new") in k[1] or ("podname", "pod-new") in k[1] for k in snap)
    finally:
        g.close()


# ---- 6 ------------------------------------------------------------------------------------
def more_slots(be: Backend):
    pods = W.make_pods(200, seed=41)
    few = W.Pods(pods.endpoints[:60], pods.ips, pods.ip_owner)
    recs = W.gen_records(30_000, pods, seed=42)
    spec = W.LOCAL_FWD_DROP + W.C5_SPEC
    g = be.engine(few, spec, False, recs, max_slots=512, max_ips=1024)
    try:
        a = Acc(g)
        be.submit(g, take(recs, slice(0, 15_000)))
        a.step()
        a.check()
        n0 = int(g.state().dense_len)
        g.load_endpoints(pods.endpoints[60:], version=2)
        assert int(g.state().dense_len) > n0  # layout_dense ran with keep
        be.submit(g, take(recs, slice(15_000, 30_000)))
        a.step()
        a.check()
        assert a.rebased == [True, False]
        assert g.delta_info()["changed_bins"] > 0
    finally:
        g.close()


# ---- 7 ------------------------------------------------------------------------------------
def reset_and_reconcile(be: Backend, spec, remote: bool):
    pods = W.make_pods(200, seed=71)
    recs = W.gen_records(30_000, pods, seed=72)
    parts = list(slices(recs, 4))
    g = be.engine(pods, spec, remote, recs)
    try:
        a = Acc(g)
        be.submit(g, parts[0])
        a.step()
        g.reset()
        be.submit(g, parts[1])
        d, reb = a.step()
        assert reb and d == a.check() and len(d) > 0
        # options equal as sets (labels reordered, entries permuted): Reconcile does nothing
        g.reconcile([dict(m, source_labels=list(reversed(m["source_labels"]))) for m in reversed(spec)])
        be.submit(g, parts[2])
        d, reb = a.step()
        assert not reb and len(d) > 0
        a.check()
        # other options: the metrics are re-created
        g.reconcile(spec[:2])
        d, reb = a.step()
        assert reb and d == {} and a.check() == {}
        be.submit(g, parts[3])
        d, reb = a.step()
        assert not reb and d == a.check() and len(d) > 0
        assert g.delta_info()["rebases"] == 3
    finally:
        g.close()


# ---- 8 ------------------------------------------------------------------------------------
def full_snapshots_between(be: Backend, name: str):
    pods, recs, spec, remote, _ = workload(name)
    g, h = be.engine(pods, spec, remote, recs), be.engine(pods, spec, remote, recs)
    try:
        a, b = Acc(g), Acc(h)
        for part in slices(recs, 3):
            be.submit(g, part)
            be.submit(h, part)
            full = g.snapshot()
            text = g.snapshot_text()
            a.step()
            assert g.snapshot() == full and g.snapshot_text() == text  # nor does a delta move the full path
            b.step()
        assert a.deltas == b.deltas and a.rebased == b.rebased == [True, False, False]
        assert a.acc == h.snapshot()
    finally:
        g.close()
        h.close()


# ---- 9 ------------------------------------------------------------------------------------
def imported(be: Backend, **kw):
    pods, recs, spec, remote, want = workload("small-wide")
    half = len(recs) // 2
    src = be.engine(pods, spec, remote, recs)
    g = be.engine(pods, spec, remote, recs, **kw)
    try:
        be.submit(src, take(recs, slice(half, len(recs))))
        ent = be.entries(src)
        a = Acc(g)
        be.submit(g, take(recs, slice(0, half)))
        a.step()
        be.import_entries(g, ent)
        _, reb = a.step()
        assert not reb
        a.check()
        got = values_only(a.acc)
        assert got == want, diff_series(got, want)
    finally:
        src.close()
        g.close()


# ---- 10 -----------------------------------------------------------------------------------
def smallest_shapes(be: Backend):
    """A 16-slot wide table (fewer slots than one wave, no growth) beside dense bins whose
    number is no multiple of 64; every occupied slot changes, then exactly one."""
    pods = W.make_pods(40, seed=5, apiserver=False)
    base = W.gen_records(400, pods, seed=6, pod_frac=1.0, drop_frac=0.5)
    verdict, ok = (base.meta >> 8) & 0xFF, base.src_ip != base.dst_ip
    rows = take(base, np.concatenate([np.flatnonzero((verdict == v) & ok)[:3] for v in (W.V_FWD, W.V_DROP)]))
    assert len(rows) == 6
    spec = W.LOCAL_FWD_DROP[:2] + [dict(m, source_labels=W.C1_LABELS) for m in W.LOCAL_FWD_DROP[2:]]
    g = be.engine(pods, spec, False, rows, max_slots=50, sparse_capacity_log2=4)
    try:
        st = g.state()
        assert int(st.sparse_len) == 16 and int(st.dense_len) % 64 != 0 and int(st.dense_len) > 0
        a = Acc(g)
        be.submit(g, rows)
        a.step()
        a.check()
        ent = be.entries(g)
        keys = len(ent)
        assert 0 < keys == len(canonical(ent)) and g.last_dropped == 0  # no duplicate slot
        info = g.delta_info()
        bins = info["changed_bins"]
        assert info["changed_entries"] == keys and bins > 0 and info["slots_scanned"] == 16
        assert info["bins_scanned"] == int(st.dense_len)
        be.submit(g, rows)  # every occupied slot and every touched bin again
        _, reb = a.step()
        a.check()
        info = g.delta_info()
        assert not reb and info["changed_entries"] == keys and info["changed_bins"] == bins, info
        one = take(rows, np.array([3]))  # one drop record towards no pod: one group-by slot, no bin
        one.dst_ip[:] = W.ip_le(100, 64, 0, 1)
        be.submit(g, one)
        d, reb = a.step()
        a.check()
        info = g.delta_info()
        assert not reb and info["changed_entries"] == 1 and info["changed_bins"] == 0, info
        assert len(d) == 2 and 1 in d.values()  # its count and bytes series
    finally:
        g.close()
