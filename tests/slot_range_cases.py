"""The slot-range cases: slot ids up to kMaxSlot = 2^21 - 2 in every structure that packs a
slot into a bit field or indexes an array by it, the u16 limit of the LDS IP images, the HLL
list geometry at its row-count limits, and the ABI's slot limits.  Written once and run on
both backends: test_slot_range_cpu.py (GPUAGG_FLAG_CPU_BACKEND, host-fed: the inputs and the
references) and test_gpu_slot_range.py (gfx950, device-resident submits, kernels by name).

Every series is compared with oracle.oracle.Module (tests.helpers), every HLL register and
estimate with oracle/sketch.py, every count-min row with it too; the decoded group-by keys
with the bit layout written out below.  Nothing is compared against the engine.

The pods of a case sit at chosen slot ids: the slots are interned in id order (namespace "n",
pod "p<id>", no owner) and gpuagg_set_endpoints installs IPs for the chosen ones alone, so the
oracle's cache holds only those pods."""

from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from oracle import oracle as O
from oracle import records as R
from oracle import sketch as S
from retina_amd import _abi
from retina_amd import workloads as W
from retina_amd.engine import Endpoint, GpuAgg, GpuAggError

from . import delta_cases
from . import dense_cases as D
from . import emit_cases
from . import sketch_cases as K
from .helpers import diff_series, dns_dict, intern_dns, oracle_cache, to_device

CPU, PER_BATCH = _abi.FLAG_CPU_BACKEND, _abi.FLAG_FOLD_PER_BATCH
U32 = np.uint32

N = (1 << 21) - 1                 # slots of the full range: ids 0 .. kMaxSlot = 2^21 - 2
CHOSEN = [0, 1, 0xFFFE, 0xFFFF, 0x10000, (1 << 17) - 1, 1 << 17, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, N - 2, N - 1]
GONE = [0xFFFF, N - 1]            # the pods the retire step takes out
OUTSIDE = [0x00000000, 0xFFFFFFFF, W.ip_le(8, 8, 8, 8)]  # addresses of no pod
SRC_PORTS, DST_PORTS = [0, 1, 443, 65535], [0, 80, 256, 65535]
HLL_EST_TOL = K.HLL_EST_TOL


class Backend:
    """device None: the CPU backend, host-fed; else that GPU, device-resident submits."""

    def __init__(self, device=None):
        self.device = device
        self.gpu = device is not None
        self.table = delta_cases.Backend(device)  # sparse_export / sparse_import buffers
        self.mem = emit_cases.Mem(device)

    @property
    def cus(self) -> int:
        return K.Backend(self.device).cus

    def create(self, spec, remote: bool, max_slots: int, flags: int = 0, **kw) -> GpuAgg:
        kw.setdefault("max_ips", 256)
        kw.setdefault("sparse_capacity_log2", 16)
        kw.setdefault("wide_list_mib", 64)  # (the default 32 GiB of lists take seconds to allocate)
        g = GpuAgg(device=self.device or 0, remote_context=remote, max_slots=max_slots,
                   flags=flags | (0 if self.gpu else CPU), **kw)
        try:
            g.reconcile(spec)
        except Exception:
            g.close()
            raise
        return g

    def submit(self, g, recs) -> None:
        if not self.gpu:
            g.submit_numpy(recs)
            return
        cols = to_device(recs, self.device)
        g.submit_device(GpuAgg.device_columns(*cols), len(recs))
        g.sync()  # (the columns are read until here)

    def see(self, g, prefix: Optional[str], what: str) -> None:
        """The aggregation kernel of the last launch, by the start of its name."""
        got = g.kernel_name()
        print("%s: %s" % (what, got if self.gpu else "(host) expects " + str(prefix)))
        if self.gpu and prefix is not None:
            assert got.startswith(prefix), (what, got, prefix)


# ---- pods at chosen slots ---------------------------------------------------------------------
def intern_range(g, lo: int, hi: int) -> None:
    """gpuagg_slot_intern of "n" / "p<i>" for i in [lo, hi): the ids come out in order."""
    fn, h, s = g.lib.gpuagg_slot_intern, g.h, C.c_int32()
    ref = C.byref(s)
    for i in range(lo, hi):
        rc = fn(h, b"n", b"p%d" % i, None, None, ref)
        if rc or s.value != i:
            g._check(rc)
            raise AssertionError("slot %d interned as %d" % (i, s.value))


@dataclass
class Placed:
    """Pods at chosen slot ids: endpoint j is "n" / "p<slots[j]>" and owns ips[j]."""
    slots: List[int]
    ips: List[List[int]]

    @property
    def pods(self) -> W.Pods:
        eps = [Endpoint("n", "p%d" % s, list(ip), None) for s, ip in zip(self.slots, self.ips)]
        flat = [x for ip in self.ips for x in ip]
        owner = [j for j, ip in enumerate(self.ips) for _ in ip]
        return W.Pods(eps, np.array(flat, U32), np.array(owner, np.int64))

    def without(self, gone: Sequence[int]) -> "Placed":
        keep = [j for j, s in enumerate(self.slots) if s not in gone]
        return Placed([self.slots[j] for j in keep], [self.ips[j] for j in keep])

    def install(self, g) -> None:
        ips = np.array([x for ip in self.ips for x in ip], U32)
        slots = np.array([s for s, ip in zip(self.slots, self.ips) for _ in ip], np.int32)
        g.set_endpoints(ips, slots)

    def slot_of(self, col: np.ndarray) -> np.ndarray:
        """The slot that owns each address, -1 for none."""
        ips = np.array([x for ip in self.ips for x in ip], U32)
        slots = np.array([s for s, ip in zip(self.slots, self.ips) for _ in ip], np.int64)
        order = np.argsort(ips)
        ips, slots = ips[order], slots[order]
        pos = np.minimum(np.searchsorted(ips, col), len(ips) - 1)
        return np.where(ips[pos] == col, slots[pos], -1)


def one_ip_each(slots: Sequence[int]) -> Placed:
    """Pod j at 10.0.0.(j + 1): one /16 prefix, one third octet -- the smallest dense radix
    image, were it not for the slot ids."""
    assert len(slots) < 250
    return Placed(list(slots), [[W.ip_le(10, 0, 0, j + 1)] for j in range(len(slots))])


def six_ips_each(slots: Sequence[int]) -> Placed:
    """Pod j at (20 + j).(1 + k).j.(7 + k), k < 6: every IP in a /16 of its own."""
    pl = Placed(list(slots), [[W.ip_le(20 + j, 1 + k, j, 7 + k) for k in range(6)] for j in range(len(slots))])
    flat = np.array([x for ip in pl.ips for x in ip], U32)
    assert len(np.unique(flat & U32(0xFFFF))) == len(flat) > 64  # kRadixMaxBlocks
    return pl


# ---- records ----------------------------------------------------------------------------------
def traffic(pl: Placed, seed: int, rounds: int = 16) -> W.Records:
    """Every (source, destination) pair of the pods' addresses and OUTSIDE, `rounds` times:
    in round r pair i takes the (source port, destination port) combination (r + i) % 16, so 16
    rounds give every pair every combination; verdict, protocol, direction, drop reason, TCP
    flags and the reply bit are seeded draws over all their values."""
    addr = np.array([x for ip in pl.ips for x in ip] + OUTSIDE, U32)
    k = len(addr)
    pair = np.arange(k * k)
    n = k * k * rounds
    combo = (np.repeat(np.arange(rounds), k * k) + np.tile(pair, rounds)) % 16
    src, dst = np.tile(addr[pair // k], rounds), np.tile(addr[pair % k], rounds)
    sport = np.array(SRC_PORTS, U32)[combo % 4]
    dport = np.array(DST_PORTS, U32)[combo // 4]
    rng = np.random.default_rng(seed)
    verdict = np.array([W.V_FWD, W.V_FWD, W.V_DROP, W.V_DROP, W.V_RETRANS, 0, 3], U32)[rng.integers(0, 7, n)]
    proto = np.array([W.PROTO_TCP, W.PROTO_TCP, W.PROTO_UDP, W.PROTO_ICMP], U32)[rng.integers(0, 4, n)]
    meta = W.pack_meta(proto, verdict, rng.integers(0, 4, n), rng.integers(0, 8, n), rng.integers(0, 64, n),
                       rng.integers(0, 2, n))
    return W.Records(src, dst, rng.integers(0, 1 << 18, n).astype(U32), meta.astype(U32),
                     (sport | (dport << U32(16))).astype(U32), np.zeros(n, U32))


def with_dns(pl: Placed, recs: W.Records, seed: int, n: int = 600) -> W.Records:
    """`recs` and n DNS queries / responses (W.gen_records) between the same pods."""
    dns = W.gen_records(n, pl.pods, seed=seed, pod_frac=0.9, drop_frac=0.0, dns_frac=1.0, n_queries=20)
    assert ((dns.meta >> 8) & 0xFF == W.V_DNS).all() and len(dns.dns) > 10
    cols = ("src_ip", "dst_ip", "bytes", "meta", "ports", "dns_id")
    return W.Records(*[np.concatenate([getattr(recs, c), getattr(dns, c)]) for c in cols], dns.dns)


def check_coverage(pl: Placed, recs: W.Records) -> None:
    """What the input has to contain, from the input: every chosen slot as a source and as a
    destination, both port extremes on both sides, both address extremes, every verdict the
    plans consume, every direction, drop reason and TCP flag combination."""
    ss, ds = pl.slot_of(recs.src_ip), pl.slot_of(recs.dst_ip)
    assert set(ss.tolist()) == set(pl.slots) | {-1} == set(ds.tolist())
    sp, dp = recs.ports & 0xFFFF, recs.ports >> 16
    for col in (sp, dp):
        assert (col == 0).any() and (col == 65535).any()
    for col in (recs.src_ip, recs.dst_ip):
        assert (col == 0).any() and (col == 0xFFFFFFFF).any()
    m = recs.meta
    verdict, tdir, reason, flags = (m >> 8) & 0xFF, (m >> 16) & 3, (m >> 18) & 7, (m >> 21) & 0x3F
    assert {W.V_FWD, W.V_DROP, W.V_RETRANS} <= set(verdict.tolist())
    assert len(np.unique(tdir)) == 4 and len(np.unique(reason[verdict == W.V_DROP])) == 8
    assert len(np.unique(flags[(verdict == W.V_FWD) & (recs.meta & 0xFF == W.PROTO_TCP)])) == 64


def oracle_run(spec, remote: bool, parts) -> dict:
    """The oracle's series after the (records, Placed) parts in order: each part is replayed
    against the cache of its own endpoint set, as the engine sees them."""
    module = O.Module(remote_context=remote)
    module.reconcile(R.spec_from_json(spec))
    for recs, pl in parts:
        b = R.Batch(recs.src_ip, recs.dst_ip, recs.bytes, recs.meta, recs.ports, recs.dns_id)
        R.replay(b, oracle_cache(pl.pods), module, dns_dict(recs))
    return module.series()


def without_pods(series: dict, gone: Sequence[int]) -> dict:
    """The series that name none of the pods `gone` in a label value."""
    names = {"p%d" % s for s in gone}
    return {k: v for k, v in series.items() if not names & {val for _, val in k[1]}}


def check(g, want: dict, what: str) -> None:
    got = g.snapshot()
    assert got == want, "%s: %s" % (what, diff_series(got, want))
    assert want and g.last_dropped == 0, what


def _m(name, src, dst=None):
    m = {"metric_name": name, "source_labels": list(src)}
    if dst is not None:
        m["destination_labels"] = list(dst)
    return m


# ---- 1. the full range ------------------------------------------------------------------------
WIDE_LABELS = ["ip", "namespace", "podname", "workload", "port"]
FWD_DROP_METRICS = ("forward_count", "forward_bytes", "drop_count", "drop_bytes")
REMOTE_FWD_DROP = [_m(x, WIDE_LABELS, WIDE_LABELS) for x in FWD_DROP_METRICS]
REMOTE_PLAN = REMOTE_FWD_DROP + [_m("tcp_flag_gauges", WIDE_LABELS, WIDE_LABELS)]
ALL_METRICS = FWD_DROP_METRICS + ("tcp_flag_gauges", "tcp_retransmission_count", "dns_request_count", "dns_response_count")
LOCAL_PLAN_A = [_m(x, ["namespace", "podname", "workload"]) for x in ALL_METRICS]
LOCAL_PLAN_B = [_m(x, ["ip", "podname", "port"]) for x in ALL_METRICS]
BINS_PER_SLOT_A = 2 * (1 + 8 + 8 + 1)  # forward, drop x 8 reasons, flags x 8, retransmit; two sides each


def full_engine(be: Backend, spec, remote: bool, **kw) -> GpuAgg:
    g = be.create(spec, remote, N, **kw)
    try:
        intern_range(g, 0, N)
    except Exception:
        g.close()
        raise
    return g


def decode_keys(ent: np.ndarray):
    """(s_slot1, d_slot1, s_port17, d_port17) of exported wide entries.  The layout
    (gpuagg_internal.h): k0 = occ:1 | group:4 | sub:6 | s_slot1:21 | s_ip:32,
    k1 = s_port17:17 | d_port17:17 | d_slot1:21 | 0:9; slot1 = slot + 1, 0 for no pod;
    port17 = 2^16 | port for TCP and UDP, 0 for the other protocols (label "unknown")."""
    k0, k1 = ent[:, 0], ent[:, 1]
    u = np.uint64
    assert (k0 >> u(63) == 1).all() and (k1 & u(0x1FF) == 0).all()
    return ((k0 >> u(32)) & u((1 << 21) - 1), (k1 >> u(9)) & u((1 << 21) - 1),
            (k1 >> u(47)) & u(0x1FFFF), (k1 >> u(30)) & u(0x1FFFF))


def implied_keys(series: dict) -> set:
    """The same tuples from the oracle's series: the pod a series names on either side is
    "p<slot>" (none: no pod), its port label the port or "unknown"."""
    out = set()
    for _, labels in series:
        lab = dict(labels)

        def side(pod, port):
            p, q = lab.get(pod, ""), lab.get(port, "")
            return (int(p[1:]) + 1 if p.startswith("p") and p[1:].isdigit() else 0, 1 << 16 | int(q) if q.isdigit() else 0)
        (s1, sp), (d1, dp) = side("source_podname", "source_port"), side("destination_podname", "destination_port")
        out.add((s1, d1, sp, dp))
    return out


@functools.lru_cache(maxsize=None)
def full_inputs():
    """The two endpoint sets of the chosen slots and three seeded batches: two over the first
    set's addresses, one over the second's."""
    a, b = one_ip_each(CHOSEN), six_ips_each(CHOSEN)
    r1, r2, r3 = traffic(a, 1), traffic(a, 2, rounds=4), traffic(b, 3, rounds=1)
    check_coverage(a, r1)
    check_coverage(b, r3)
    return a, b, r1, r2, r3


def full_range_remote(be: Backend) -> None:
    a, b, r1, r2, r3 = full_inputs()
    g = full_engine(be, REMOTE_FWD_DROP, True, sparse_capacity_log2=4)
    try:
        g._check(g.lib.gpuagg_set_sparse_growth(g.h, 20, 0))
        a.install(g)
        # 1. wide keys on both sides from a 16-slot table: overflow list, regrow, replay.  The
        #    forward / drop plan alone is what wide_kernel takes (no tcpflags group) ...
        be.submit(g, r1)
        be.see(g, "wide_kernel<", "remote, forward + drop")
        check(g, oracle_run(REMOTE_FWD_DROP, True, [(r1, a)]), "remote, forward + drop")
        assert g.sparse_info()["grows"] >= 1, g.sparse_info()
        # ... and with tcp_flag_gauges (the flag index in the key's sub field) aggregate_kernel
        g.reconcile(REMOTE_PLAN)
        be.submit(g, r1)
        be.see(g, "aggregate_kernel<", "remote, with tcp flags")
        want1 = oracle_run(REMOTE_PLAN, True, [(r1, a)])
        check(g, want1, "remote, with tcp flags")
        assert g.sparse_info()["grows"] >= 1, g.sparse_info()
        # 2. the exported keys, decoded here; reset, import, the same snapshot
        ent = be.table.entries(g)
        got = set(zip(*[x.tolist() for x in decode_keys(ent)]))
        want_keys = implied_keys(want1)
        assert got == want_keys, (sorted(got - want_keys)[:5], sorted(want_keys - got)[:5])
        top = max(CHOSEN) + 1
        assert {k[0] for k in got} >= {top, 0} and {k[1] for k in got} >= {top, 0}
        assert {0, 1 << 16, 0x1FFFF} <= {k[2] for k in got} and {0, 1 << 16, 0x1FFFF} <= {k[3] for k in got}
        g.reset()
        be.table.import_entries(g, ent)
        check(g, want1, "remote, imported")
        # 3. deltas: the first rebased, their sum the snapshot
        acc = delta_cases.Acc(g)
        acc.step()
        be.submit(g, r2)
        acc.step()
        assert acc.rebased == [True, False]
        want2 = oracle_run(REMOTE_PLAN, True, [(r1, a), (r2, a)])
        assert acc.check() == want2, diff_series(acc.acc, want2)
        # 4. 72 IPs in 72 /16 prefixes: the bucket hash table, not the radix blocks
        b.install(g)
        be.submit(g, r3)
        want3 = oracle_run(REMOTE_PLAN, True, [(r1, a), (r2, a), (r3, b)])
        check(g, want3, "remote, second endpoint set")
        # 5. retire everything but ten pods
        b.without(GONE).install(g)
        assert g.retire_slots() == N - 10
        want5 = without_pods(want3, GONE)
        assert len(want5) < len(want3)
        check(g, want5, "remote, retired")
        free = np.setdiff1d(np.arange(N), np.array(b.without(GONE).slots))
        assert g.slot_intern("n", "another") == int(free.min()) == 2
    finally:
        g.close()


def hll_rows(pl: Placed, parts: Sequence[W.Records], p: int) -> dict:
    """{slot: its 2^p registers} of the pods that are a source, from oracle.sketch.hll_update."""
    slots = sorted(pl.slots)
    regs = np.zeros((len(slots), 1 << p), np.uint8)
    for r in parts:
        s = pl.slot_of(r.src_ip)
        S.hll_update(regs, np.where(s >= 0, np.searchsorted(slots, s), -1), r.dst_ip, p)
    return {s: regs[j] for j, s in enumerate(slots) if regs[j].any()}


def check_hll(g, want: dict, rows: int, p: int, what: str) -> np.ndarray:
    """The whole register array and every estimate: the rows of `want` equal, all others 0."""
    hll = g.hll_array()
    assert hll.shape == (rows, 1 << p), (what, hll.shape)
    used = np.flatnonzero(hll.any(axis=1))
    assert used.tolist() == sorted(want), (what, used[:20].tolist(), sorted(want))
    for s, regs in want.items():
        assert np.array_equal(hll[s], regs), (what, s)
    est = g.hll_estimates()
    assert est.shape == (rows,)
    for s, regs in want.items():
        w = S.hll_estimate(regs)
        assert abs(est[s] - w) <= HLL_EST_TOL * w, (what, s, est[s], w)
    rest = np.ones(rows, bool)
    rest[sorted(want)] = False
    assert (est[rest] == 0.0).all(), what
    return hll


def full_range_local(be: Backend) -> None:
    a, b, r1, _, _ = full_inputs()
    recs = with_dns(a, r1, 4)
    p = 4
    g = full_engine(be, LOCAL_PLAN_A, False, hll_precision=p, sparse_capacity_log2=16)
    try:
        a.install(g)
        intern_dns(g, recs)
        # 1. dense bins of every slot, compact DNS keys; the LDS image refused
        assert int(g.state().dense_len) == BINS_PER_SLOT_A * N == 75_497_436
        assert -(-int(g.state().dense_len) // D.FOLD_WINDOW_BINS) > D.MAX_SPILL_WINDOWS
        be.submit(g, recs)
        be.see(g, "dense_local_kernel<", "local, plan A")
        sk = g.sketch_kernel_name()
        check(g, oracle_run(LOCAL_PLAN_A, False, [(recs, a)]), "local, plan A")
        # 2. HLL: ceil(N / 256) = 8192 fine windows, the last of 255 pods; 16 super-windows
        geo = hll_shape(p, N, len(recs), be.cus)
        assert -(-N // 256) == 8192 and N % 256 == 255 and (geo["hsshift"], geo["hnsup"]) == (17, 16)
        want_h = hll_rows(a, [recs], p)
        assert sorted(want_h) == sorted(CHOSEN)
        check_hll(g, want_h, N, p, "local, plan A")
        print("sketch pass:", sk or "(host)")
        if be.gpu:  # lists, so the staged scatter kernel (the folds are not part of the name)
            assert sk.startswith("sketch_stage_kernel<"), sk
        # 3. enrichment of every address
        addr = np.array([x for ip in a.ips for x in ip] + OUTSIDE, U32)
        gs, gd = emit_cases.run_enrich(g, be.mem, addr, addr[::-1].copy())
        assert gs.tolist() == CHOSEN + [-1, -1, -1] and gd.tolist() == gs[::-1].tolist()
        # 4. wide keys in local context
        g.reconcile(LOCAL_PLAN_B)
        be.submit(g, recs)
        be.see(g, "aggregate_kernel<", "local, plan B")
        want_b = oracle_run(LOCAL_PLAN_B, False, [(recs, a)])
        check(g, want_b, "local, plan B")
        hll = check_hll(g, want_h, N, p, "local, plan B")
        # 5. retire
        a.without(GONE).install(g)
        assert g.retire_slots() == N - 10
        check(g, without_pods(want_b, GONE), "local, retired")
        kept = {s: r for s, r in want_h.items() if s not in GONE}
        after = check_hll(g, kept, N, p, "local, retired")
        assert not after[GONE].any() and np.array_equal(after[sorted(kept)], hll[sorted(kept)])
    finally:
        g.close()


# ---- 2. the u16 limit of the LDS images ---------------------------------------------------------
U16_LAST, U16_FIRST_REFUSED = 0xFFFE, 0xFFFF  # kIplNoSlot = 0xFFFF marks "no pod" in an image
BELOW = [0, 0x7FFF, 0x8000, 0xFFFD, U16_LAST]
U16_MAX_SLOTS = 65_600
# id -> (spec, remote, sketch geometry)
U16_PLANS = {"local": (W.LOCAL_FWD_DROP, False, {}), "remote": (W.C1_REMOTE, True, {}),
             "sketch": (W.LOCAL_FWD_DROP, False, dict(cms_depth=2, cms_width_log2=12, hll_precision=8))}


def u16_names(plan: str, pl: Placed, n_slots: int):
    """(aggregation kernel, its start suffices; sketch scatter kernel) the planner model gives
    for pods at these slots."""
    spec, remote, sk = U16_PLANS[plan]
    image = max(pl.slots) < U16_FIRST_REFUSED
    if remote:  # wide_kernel<ng, opt, excl, kip>: kip -1 without the image of every pod IP
        name = "wide_kernel<2, true, true, %d>" % (2 if image else -1)
    else:
        geo = D.geometry(spec, pl.pods, n_slots=n_slots, max_slot=max(pl.slots))
        assert geo.tier1 == image
        name = D.kernel_name(geo)
        assert name.startswith("dense_lds_kernel<" if image else "dense_local_kernel<"), name
    sketch = stage_name(pl) if sk else None
    return name, sketch


def stage_name(pl: Placed) -> str:
    """sketch_stage_kernel<kIp, kD> of a pass with HLL lists and a count-min depth other than 4:
    kIp 3, the dense radix image that one_ip_each's addresses take, while every installed slot
    is below 0xFFFF; else 0, the HBM table."""
    return "sketch_stage_kernel<%d, 0>" % (3 if max(pl.slots) < U16_FIRST_REFUSED else 0)


@functools.lru_cache(maxsize=None)
def u16_records(slots: tuple, seed: int):
    pl = one_ip_each(slots)
    return pl, traffic(pl, seed, rounds=16)


def check_sketches(g, pl: Placed, recs: W.Records, rows: int, d: int, w: int, p: int, what: str) -> None:
    cms = np.zeros((d, 1 << w), np.uint32)
    S.cms_update(cms, recs.src_ip, recs.dst_ip, recs.ports, recs.meta & U32(0xFF))
    assert np.array_equal(g.cms_array(), cms), what
    check_hll(g, hll_rows(pl, [recs], p), rows, p, what)


def u16_step(be: Backend, g, plan: str, pl: Placed, recs, n_slots: int, rows: int, what: str) -> None:
    """One reset, install, submit and compare; the kernels by name."""
    spec, remote, sk = U16_PLANS[plan]
    name, sketch = u16_names(plan, pl, n_slots)
    g.reset()
    pl.install(g)
    be.submit(g, recs)
    be.see(g, name, what)
    got = g.sketch_kernel_name()
    check(g, oracle_run(spec, remote, [(recs, pl)]), what)
    if sk:
        check_sketches(g, pl, recs, rows, sk["cms_depth"], sk["cms_width_log2"], sk["hll_precision"], what)
        print("%s: %s" % (what, got or "(host) expects " + sketch))
        if be.gpu:
            assert got == sketch, (what, got, sketch)


def u16_limit(be: Backend, plan: str) -> None:
    """Slot 0xFFFE is the last an image holds; with 0xFFFF installed the HBM table serves."""
    spec, remote, sk = U16_PLANS[plan]
    g = be.create(spec, remote, U16_MAX_SLOTS, **sk)
    try:
        intern_range(g, 0, U16_FIRST_REFUSED)
        pl, recs = u16_records(tuple(BELOW), 5)
        u16_step(be, g, plan, pl, recs, U16_FIRST_REFUSED, 1 << 16, "%s, slots <= 0xFFFE" % plan)
        intern_range(g, U16_FIRST_REFUSED, U16_FIRST_REFUSED + 1)
        pl, recs = u16_records(tuple(BELOW + [U16_FIRST_REFUSED]), 6)
        u16_step(be, g, plan, pl, recs, U16_FIRST_REFUSED + 1, 1 << 16, "%s, slot 0xFFFF" % plan)
    finally:
        g.close()


REUSE_SLOTS = [0xFFFF, 0x10000, 0x10001, U16_MAX_SLOTS - 2, U16_MAX_SLOTS - 1]


def u16_retire_reuse(be: Backend) -> None:
    """205 endpoints ever, five live: the count of pods says "image", the slot ids refuse it."""
    spec = W.LOCAL_FWD_DROP
    g = be.create(spec, False, U16_MAX_SLOTS)
    try:
        intern_range(g, 0, U16_MAX_SLOTS)
        first = one_ip_each(range(200))
        first.install(g)
        pl, recs = u16_records(tuple(REUSE_SLOTS), 7)
        pl.install(g)  # the first 200 are deleted ...
        assert g.retire_slots() == U16_MAX_SLOTS - len(REUSE_SLOTS)  # ... and retired with the never-installed
        assert len(first.slots) + len(pl.slots) < U16_FIRST_REFUSED <= min(pl.slots)
        geo = D.geometry(spec, pl.pods, n_slots=U16_MAX_SLOTS, max_slot=max(pl.slots))
        assert not geo.tier1 and D.geometry(spec, pl.pods, n_slots=U16_MAX_SLOTS).tier1
        assert int(g.state().dense_len) == geo.dense_len
        be.submit(g, recs)
        be.see(g, D.kernel_name(geo), "retired and reused")
        assert D.kernel_name(geo).startswith("dense_local_kernel<")
        check(g, oracle_run(spec, False, [(recs, pl)]), "retired and reused")
    finally:
        g.close()


# ---- 3. HLL row-count limits --------------------------------------------------------------------
# id -> (precision, slots interned, max_slots, lists)
HLL_ROWS = {
    "p17-8192": (17, 8192, 8192, True),      # hnwin = 8192 = kHllMaxWindows, one pod a window, nfine 512
    "p17-8256": (17, 8256, 8256, False),     # hnwin > 8192: direct CAS
    "p10-70016": (10, 70_016, 70_016, True),  # 547 windows, nfine 64, rows beyond 0xFFFF
    "p10-2112": (10, 2112, 2112, True),      # 17 windows: the first shape with hsshift > hshift
    "p10-2048": (10, 2048, 2048, True),      # 16 windows: hsshift == hshift
    "p4-4150": (4, 4160, 4150, True),        # 17 windows, the last of 54 pods
}
HLL_MAX_WINDOWS = 8192
HLL_N = 20_000


def hll_shape(p: int, rows: int, n: int, cus: int):
    """hshift and the number of fine windows beside sketch_cases.list_geometry; lists: what
    sketch_geom (gpuagg_sketch_plan.h) decides (hnwin <= kHllMaxWindows and hnsup <= 1024)."""
    geo = K.list_geometry(n, cus, 1, 15, p, rows)  # (its count-min part is not used)
    geo["hshift"] = min(8, 17 - p)
    geo["hnwin"] = -(-rows >> geo["hshift"])
    geo["lists"] = geo["hnwin"] <= HLL_MAX_WINDOWS and geo["hnsup"] <= 1024
    return geo


def hll_sources(rows: int, geo) -> List[int]:
    """The first and last row of the first, a middle and the last fine window, and the first
    row of the last super-window (the first super-window starts at row 0)."""
    f, nwin = 1 << geo["hshift"], geo["hnwin"]
    out = set()
    for w in (0, nwin // 2, nwin - 1):
        out |= {w * f, min(rows, (w + 1) * f) - 1}
    out.add((geo["hnsup"] - 1) << geo["hsshift"])
    assert max(out) == rows - 1 and min(out) == 0
    return sorted(out)


def hll_records(pl: Placed, n: int, seed: int) -> W.Records:
    """Sources: the pods and one address of no pod; destinations: seeded, mostly distinct."""
    rng = np.random.default_rng(seed)
    addr = np.array([ip[0] for ip in pl.ips] + [OUTSIDE[2]], U32)
    src = addr[rng.integers(0, len(addr), n)]
    dst = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)
    return W.Records(src, dst, np.full(n, 64, U32), np.full(n, W.pack_meta(W.PROTO_TCP, W.V_FWD, 1), U32),
                     np.full(n, 40000 | (443 << 16), U32), np.zeros(n, U32))


def busiest_hll_list(pl: Placed, recs: W.Records, geo, cus: int) -> int:
    """Entries of the fullest level-1 list: per scatter workgroup and super-window."""
    slot = pl.slot_of(recs.src_ip)
    wg = np.arange(len(recs), dtype=np.int64) // geo["chunk"]
    assert int(wg[-1]) < cus
    ok = slot >= 0
    return int(np.bincount(wg[ok] * geo["hnsup"] + (slot[ok] >> geo["hsshift"]), minlength=cus * geo["hnsup"]).max())


def hll_engine(be: Backend, p: int, interned: int, max_slots: int) -> GpuAgg:
    g = be.create(K.SPEC, False, max_slots, flags=PER_BATCH, hll_precision=p)
    try:
        intern_range(g, 0, min(interned, max_slots))
    except Exception:
        g.close()
        raise
    return g


def hll_row_limits(be: Backend, which: str) -> None:
    p, interned, max_slots, lists = HLL_ROWS[which]
    rows = min(interned, max_slots)
    geo = hll_shape(p, rows, HLL_N, be.cus)
    assert geo["lists"] == lists, geo
    nfine = 1 << (geo["hsshift"] - geo["hshift"])
    assert (geo["hnwin"], nfine) == {"p17-8192": (8192, 512), "p17-8256": (8256, 512), "p10-70016": (547, 64),
                                     "p10-2112": (17, 2), "p10-2048": (16, 1), "p4-4150": (17, 2)}[which], geo
    if which == "p4-4150":
        assert rows - ((geo["hnwin"] - 1) << geo["hshift"]) == 54
    pl = one_ip_each(hll_sources(rows, geo))
    if which == "p10-70016":
        assert max(pl.slots) > 0xFFFF
    recs = hll_records(pl, HLL_N, 8)
    if lists:  # the lists carry every update: none reaches its capacity
        busiest = busiest_hll_list(pl, recs, geo, be.cus)
        print("busiest HLL list %d of capacity %d; %s" % (busiest, geo["hcap"], geo))
        assert busiest <= geo["hcap"], (busiest, geo)
    g = hll_engine(be, p, interned, max_slots)
    try:
        pl.install(g)
        assert int(g.state().hll_len) >> p == rows
        be.submit(g, recs)
        name = g.sketch_kernel_name()
        print("%s: %s" % (which, name or "(host)"))
        want = hll_rows(pl, [recs], p)
        assert sorted(want) == sorted(pl.slots)
        check_hll(g, want, rows, p, which)
        assert "hll_split_kernel" not in name or lists
        if be.gpu:  # lists: the staged scatter kernel; none: every update a CAS from the unstaged one
            assert name == (stage_name(pl) if lists else "sketch_scatter_kernel<true, false>"), name
    finally:
        g.close()


HLL_OVERFLOW_N = 100_000


def hll_list_overflow(be: Backend) -> None:
    """p = 10, 2,112 rows, every source pod in super-window 0: each workgroup's chunk goes to
    one list of 9, which holds a third of it; the rest takes the full-list CAS."""
    p, rows = 10, 2112
    geo = hll_shape(p, rows, HLL_OVERFLOW_N, be.cus)
    assert (geo["hsshift"], geo["hnsup"]) == (8, 9)
    pl = one_ip_each([0, 1, 127, 128, 255])
    assert max(pl.slots) >> geo["hsshift"] == 0
    recs = hll_records(pl, HLL_OVERFLOW_N, 9)
    busiest = busiest_hll_list(pl, recs, geo, be.cus)
    print("busiest HLL list %d of capacity %d; %s" % (busiest, geo["hcap"], geo))
    assert busiest >= 2 * geo["hcap"], (busiest, geo)
    g = hll_engine(be, p, rows, rows)
    try:
        pl.install(g)
        be.submit(g, recs)
        name = g.sketch_kernel_name()
        print("overflow: %s" % (name or "(host)"))
        check_hll(g, hll_rows(pl, [recs], p), rows, p, "overflow")
        if be.gpu:
            assert name == stage_name(pl), name
    finally:
        g.close()


# ---- 4. ABI limits ------------------------------------------------------------------------------
def code_of(fn) -> int:
    try:
        fn()
    except GpuAggError as e:
        return e.code
    return _abi.OK


def abi_max_slots(be: Backend) -> None:
    be.create([], False, N).close()
    assert code_of(lambda: be.create([], False, N + 1)) == _abi.EINVAL


def abi_capacity_and_reuse(be: Backend) -> None:
    g = be.create(W.LOCAL_FWD_DROP, False, 3)
    try:
        intern_range(g, 0, 3)
        assert code_of(lambda: g.slot_intern("n", "p3")) == _abi.ECAPACITY
        pl = one_ip_each([0, 1, 2])
        pl.install(g)
        pl.without([1]).install(g)
        assert g.retire_slots() == 1
        assert g.slot_intern("n", "p3") == 1
    finally:
        g.close()


def abi_refused_endpoints(be: Backend) -> None:
    """A never-interned, a negative and a retired slot: EINVAL each, and the installed table
    still answers."""
    g = be.create(W.LOCAL_FWD_DROP, False, 64)
    try:
        intern_range(g, 0, 4)
        pl = one_ip_each([0, 1, 2, 3])
        pl.install(g)
        kept = pl.without([3])
        kept.install(g)
        assert g.retire_slots() == 1
        ip = np.array([W.ip_le(10, 9, 9, 9)], U32)
        for bad in (4, 63, 64, -1, 3):
            assert code_of(lambda: g.set_endpoints(ip, np.array([bad], np.int32))) == _abi.EINVAL, bad
        recs = traffic(kept, 10, rounds=1)
        be.submit(g, recs)
        check(g, oracle_run(W.LOCAL_FWD_DROP, False, [(recs, kept)]), "after refused installs")
        addr = np.array([x[0] for x in pl.ips] + [int(ip[0])], U32)
        gs, _ = emit_cases.run_enrich(g, be.mem, addr, addr)
        assert gs.tolist() == [0, 1, 2, -1, -1]
    finally:
        g.close()
