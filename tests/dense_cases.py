"""The dense-counter cases (launch_aggregate: dense_lds_kernel, dense_local_kernel, the spill
lists, spill_window_kernel, stage_reduce_kernel), written once and run on both backends:
test_dense_cases_cpu.py (GPUAGG_FLAG_CPU_BACKEND, host-fed: the inputs, the references and the
restated geometry against the host mirror) and test_gpu_dense_cases.py (gfx950,
device-resident submits, every kernel asserted by name).

What every case asserts: every series (name, label values, exact integer value) against a
reference that never comes from the engine -- oracle.oracle.Module per flow up to 50,000
records, the C port (oracle.ref_cpu.RefCPU) above, and for the hot-bin inputs the reference
of the distinct records times their multiplicity --; the geometry the case is there for,
restated from gpuagg_state().dense_len and the constants below (`geometry`); and -- on the
GPU -- gpuagg_kernel_name() against `kernel_name`, the Python restatement of the launcher's
variant selection.  Each case prints the name it saw."""

from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from oracle.ref_cpu import values_only
from retina_amd import _abi
from retina_amd import workloads as W

from .growth_inputs import ref_series, scale_series, slices, take
from .helpers import diff_series, make_engine, oracle_series, to_device

CPU, PER_BATCH, NO_LDS_IP = _abi.FLAG_CPU_BACKEND, _abi.FLAG_FOLD_PER_BATCH, _abi.FLAG_NO_LDS_IP_TABLE
CUCKOO, ROW_RADIX = _abi.FLAG_LDS_CUCKOO, _abi.FLAG_ROW_RADIX  # the LDS IP image's other forms (kIp 0, 1)

# ---- geometry facts (each restates the line of the sources it names) ------------------------
LDS_BYTES = 160 * 1024                              # gpuagg_internal.h: kLdsBytes
MAX_SPILL_WINDOWS = 256                             # kMaxSpillWindows
SPILL_RING = 128                                    # kSpillRing
L4_EXTRA_BYTES = 64 * 4 + MAX_SPILL_WINDOWS * 4     # kL4ExtraBytes: dummies + spill counters
TIER1_MAX_BINS = (LDS_BYTES - L4_EXTRA_BYTES) // 4  # u32 bins of tier 1 with no IP image: 40,640
LDS_EXTRA_WORDS = 64 + MAX_SPILL_WINDOWS // 2       # kLdsExtraWords
TIER2_MAX_BINS = LDS_BYTES // 8 - LDS_EXTRA_WORDS   # kLdsMaxBins: 20,288 u64 bins
FOLD_WINDOW_SHIFT = 13                              # kFoldWindowShift
FOLD_WINDOW_BINS = 1 << FOLD_WINDOW_SHIFT           # 8,192 bins per spill window
ENTRY_BYTES_LIMIT = 1 << (31 - FOLD_WINDOW_SHIFT)   # DenseSink::entry: a plain entry carries < 2^18 bytes
L4_COUNT_LIMIT, L4_BYTE_LIMIT = 1 << 12, 1 << 20    # tier-1 LDS word: count:12 | bytes:20 (kL4CountShift)
Q_BYTES = (1 << 29) - 1                             # dense_lds_kernel: kQBytes of the C2 drop queue
FOLD_EXACT_ENTRIES = 1 << 20                        # spill_window_kernel: fast = total < 2^20
FOLD_WAVE_PER_LIST = 2048                           # spill_window_kernel: total < lists_here * 2048
IPL_MAX_BYTES = 112 * 1024                          # kIplMaxBytes
SPARSE_SEG_LOG2 = 13                                # kSparseSegLog2 (compact keys)
MAX_RECORDS_PER_BLOCK = (1 << 20) - 4               # kMaxRecordsPerBlock
DEFER_LAUNCHES, SMALL_LAUNCH_CHUNK = 64, 1 << 16    # gpuagg_runtime.cpp: kDeferLaunches, kSmallLaunchChunk
SPARSE_CAPACITY_LOG2 = 20                           # helpers.make_engine's default
# a residency the cases rely on is decided at least this many bins away from the LDS limit
# (the tier-1 image leaves the apiserver pseudo pod out: at most one 256-address block of
# 128 words less than `ipl_dense_bytes` says)
MARGIN = 256

FAM_FWD, FAM_DROP, FAM_TCPFLAGS, FAM_RETRANS, FAM_DNS_REQ, FAM_DNS_RESP = range(6)
FAMILY = {"forward_count": FAM_FWD, "forward_bytes": FAM_FWD, "drop_count": FAM_DROP, "drop_bytes": FAM_DROP,
          "tcp_flag_gauges": FAM_TCPFLAGS, "tcp_retransmission_count": FAM_RETRANS,
          "dns_request_count": FAM_DNS_REQ, "dns_response_count": FAM_DNS_RESP}
PRIO = (0, 2, 1, 3, 9, 9)  # gpuagg_reconcile: layout order forward, tcpflags, drop, retransmit
EP_LABELS = frozenset(["namespace", "podname", "workload"])  # OPT_EP: read from the endpoint


def sig_group(fam: int, in_lds: bool) -> int:
    """gpuagg_internal.h sig_group: 4 bits per group, family + 1 | in-LDS << 3."""
    return (fam + 1) | (8 if in_lds else 0)


SIG_FWD_LDS = sig_group(FAM_FWD, True)                                      # 9
SIG_FWD_LDS_DROP_LDS = SIG_FWD_LDS | sig_group(FAM_DROP, True) << 4         # 169
SIG_FWD_LDS_DROP_SPILL = SIG_FWD_LDS | sig_group(FAM_DROP, False) << 4      # 41: C2's production signature
SIG_C5 = (sig_group(FAM_TCPFLAGS, False) | sig_group(FAM_RETRANS, False) << 4 |
          sig_group(FAM_DNS_REQ, False) << 8 | sig_group(FAM_DNS_RESP, False) << 12)  # 25923
assert (SIG_FWD_LDS, SIG_FWD_LDS_DROP_LDS, SIG_FWD_LDS_DROP_SPILL, SIG_C5) == (9, 169, 41, 25923)


@dataclass
class Group:
    fam: int
    labels: frozenset
    sparse: bool   # the DNS groups: compact keys, no dense bins
    keyed: bool    # key_mode: bins per pod; else the keyless group of 2 * nsub bins
    nsub: int
    base: int = 0
    nbins: int = 0
    in_lds: bool = False

    @property
    def end(self) -> int:
        return self.base + self.nbins


def plan_groups(spec) -> List[Group]:
    """gpuagg_reconcile: one group per (family, labels) in the registry's order -- a map keyed
    by metric name --, then dense groups by PRIO (stable) and the DNS groups behind them."""
    out: List[Group] = []
    for m in sorted(spec, key=lambda m: m["metric_name"]):
        fam, labels = FAMILY[m["metric_name"]], frozenset(m["source_labels"])
        if not labels or any(g.fam == fam and g.labels == labels for g in out):
            continue
        out.append(Group(fam, labels, fam >= FAM_DNS_REQ, bool(labels & EP_LABELS),
                         8 if fam in (FAM_DROP, FAM_TCPFLAGS) else 1))
    return sorted(out, key=lambda g: (g.sparse, 0 if g.sparse else PRIO[g.fam]))


def key_cap_for(n_slots: int) -> int:
    """key_cap_for: the slots in use rounded up to 64 (max_slots is never the smaller here)."""
    return max(64, (n_slots + 63) & ~63)


def ipl_dense_bytes(pods) -> int:
    """iprd_build: one 256-address block of u16 slots per third octet of each /16 prefix's run
    [min, max], plus the "no pod" block."""
    pfx, o3 = pods.ips & np.uint32(0xFFFF), (pods.ips >> np.uint32(16)) & np.uint32(0xFF)
    nblk = sum(int(o3[pfx == p].max()) - int(o3[pfx == p].min()) + 1 for p in np.unique(pfx))
    return (nblk + 1) * 512


def ipl_bytes_range(pods, kip: int):
    """(least, most) bytes of the tier-1 LDS IP image in form kip.  2: iprd_build's dense image,
    exact.  1: ipr_build -- the row table of (npfx + 1) * 256 u16 (npfx <= kIprMaxPfx = 4) and
    one block per populated third octet, at most the dense image's blocks.  0: ipl_build --
    nb buckets of two (u32 key, u16 slot) entries at 88 % load, nb growing by 1/16 every 8 of
    at most 96 attempts (less than twice).  The forms other than 2 are bounded, not restated:
    a residency has to hold for every size in the range."""
    dense = ipl_dense_bytes(pods)
    if kip == 2:
        return dense, dense
    if kip == 1:
        return 0, dense + 5 * 512
    nb = -(-len(pods.ips) * 100 // (88 * 2))
    return 0, 2 * (((nb * 8 + 15) & ~15) + ((nb * 4 + 2 + 15) & ~15)) + 64


@dataclass
class Geometry:
    groups: List[Group]
    dense_len: int
    tier1: bool
    dns: bool
    L: int           # bins of the LDS prefix
    sig: int
    nwin: int        # spill windows behind the prefix; 0: no lists (none needed, or more than 256)
    windows: int     # ceil((dense_len - L) / 8192)
    seg_lists: int   # compact-key segment lists (their fill counters take LDS words in tier 2)
    kip: int = 2     # form of the tier-1 LDS IP image: 0 cuckoo, 1 row radix, 2 dense radix

    def dense(self) -> List[Group]:
        return [g for g in self.groups if not g.sparse]


def image_holds(pods, max_slot: Optional[int] = None) -> bool:
    """ipl_build.h: an LDS image holds u16 slots with 0xFFFF for "no pod", so the largest
    installed slot id decides -- the pods' count stands for it where slots are never reused."""
    return (len(pods.endpoints) if max_slot is None else max_slot) < 0xFFFF


def geometry(spec, pods, flags: int = 0, n_slots: Optional[int] = None, max_slot: Optional[int] = None) -> Geometry:
    """aggregate() restated: the layout, the tier, the LDS prefix of whole groups, the kernel
    signature and the spill windows.  Asserts that every residency is decided with MARGIN.
    n_slots: the slots interned (default: one per pod, ids 0 ..); max_slot: the largest
    installed slot id (`image_holds`)."""
    gs = plan_groups(spec)
    kc, total = key_cap_for(len(pods.endpoints) if n_slots is None else n_slots), 0
    for g in gs:
        if not g.sparse:
            g.base, g.nbins = total, (kc if g.keyed else 1) * 2 * g.nsub
            total = g.end
    dense = [g for g in gs if not g.sparse]
    dns = any(g.sparse for g in gs)
    kip = 0 if flags & CUCKOO else 1 if flags & ROW_RADIX else 2  # build_lds_image
    ipl_lo, ipl_hi = ipl_bytes_range(pods, kip)
    tier1 = bool(dense) and not dns and not flags & NO_LDS_IP and ipl_hi <= IPL_MAX_BYTES and image_holds(pods, max_slot)
    seg = (1 << SPARSE_CAPACITY_LOG2) >> SPARSE_SEG_LOG2 if dns else 0
    # the limit with the largest and with the smallest image (one number but for kIp 0 / 1)
    lo, hi = [(LDS_BYTES - b - L4_EXTRA_BYTES) // 4 if tier1 else TIER2_MAX_BINS - (seg + 1) // 2 for b in (ipl_hi, ipl_lo)]
    L = 0
    for g in dense:
        assert g.end <= lo - MARGIN or g.end >= hi + MARGIN, "group ends at %d, within %d bins of the LDS limit %d..%d" % (
            g.end, MARGIN, lo, hi)
        if g.end > lo:
            break
        g.in_lds, L = True, g.end
    sig = 0
    if len(gs) <= 8 and (tier1 or (dns and dense)):
        for i, g in enumerate(gs):
            sig |= sig_group(g.fam, g.in_lds) << (4 * i)
    windows = -(-(total - L) // FOLD_WINDOW_BINS)
    return Geometry(gs, total, tier1, dns, L, sig, windows if windows <= MAX_SPILL_WINDOWS else 0, windows, seg, kip)


def kernel_name(geo: Geometry, vec: bool = True) -> str:
    """launch_aggregate's variant, as gpuagg_kernel_name() prints it; the tier-1 names end with
    the LDS IP image's form (2: the dense radix image that make_pods' addresses take unflagged)."""
    kip = geo.kip
    ng = next(x for x in (1, 2, 4, 8) if len(geo.groups) <= x)
    v = "true" if vec else "false"
    if geo.tier1:  # variants 200 / 201 / 202 carry their signature, 101 .. 108 the group count
        if geo.sig in (SIG_FWD_LDS, SIG_FWD_LDS_DROP_LDS, SIG_FWD_LDS_DROP_SPILL):
            return "dense_lds_kernel<%d, %s, %du, %d>" % (1 if geo.sig == SIG_FWD_LDS else 2, v, geo.sig, kip)
        return "dense_lds_kernel<%d, %s, 0u, %d>" % (ng, v, kip)
    c5 = geo.dns and ng == 4 and geo.sig == SIG_C5  # variant 305; 306 when the rings fit
    lds = (geo.L + LDS_EXTRA_WORDS) * 8 + geo.seg_lists * 4
    staged = c5 and geo.nwin and lds + geo.nwin * (1 + SPILL_RING) * 4 <= LDS_BYTES
    return "dense_local_kernel<%d, %s, %s, %du%s>" % (ng, v, "true" if geo.dns else "false",
                                                       geo.sig if c5 else 0, ", true" if staged else "")


def launch_chunk(n: int, blocks: int) -> int:
    """aggregate(): records per workgroup."""
    return ((n + blocks - 1) // blocks + 3) & ~3


def spill_cap(geo: Geometry, chunk: int, per_batch: bool) -> int:
    """aggregate()'s geom(): entries per (workgroup, window) list.  Deferred folds size the
    lists for up to kDeferLaunches launches of this chunk."""
    budget = chunk if per_batch else max(chunk, min(MAX_RECORDS_PER_BLOCK, DEFER_LAUNCHES * chunk))
    return ((2 * budget // geo.nwin + 4096) + 3) & ~3


def fold_partitions(geo: Geometry, blocks: int):
    """launch_folds: (partitions per window, lists of a partition at most)."""
    nparts = max(1, 2 * blocks // geo.nwin)
    return nparts, -(-blocks // nparts)


# ---- backend ------------------------------------------------------------------------------
class Backend:
    """device None: the CPU backend, host-fed; else that GPU, device-resident submits."""

    def __init__(self, device=None):
        self.device = device
        self.gpu = device is not None

    @property
    def cus(self) -> int:
        """Workgroups of a dense launch (one per CU); the host mirror has none: 256."""
        if not self.gpu:
            return 256
        import torch
        return int(torch.cuda.get_device_properties(self.device).multi_processor_count)

    def engine(self, pods, spec, flags=0, recs=None, **kw):
        if not self.gpu:
            return make_engine(pods, spec, False, recs=recs, flags=CPU | flags, **kw)
        return make_engine(pods, spec, False, self.device, recs, flags=flags, **kw)

    def submit(self, g, recs, unaligned=False):
        """One unsynced submit.  unaligned True: every column starts one element past a
        16-byte boundary; "bytes": that column alone.  Returns what has to stay alive until
        the engine has read it."""
        names = ("src_ip", "dst_ip", "bytes", "meta", "ports", "dns_id")
        off = [bool(unaligned) and (unaligned is True or unaligned == k) for k in names]
        if not self.gpu:
            cols = [np.concatenate([np.zeros(1, a.dtype), a])[1:] if o else a
                    for o, a in zip(off, (getattr(recs, k) for k in names))]
            g.submit_numpy(W.Records(*cols))
            return None
        import torch
        from retina_amd import GpuAgg
        ts = [torch.cat([t.new_zeros(1), t])[1:] if o else t for o, t in zip(off, to_device(recs, self.device))]
        assert all(t.data_ptr() % 16 == (4 if o else 0) for o, t in zip(off, ts))
        g.submit_device(GpuAgg.device_columns(*ts), len(recs))
        return ts


# ---- references -----------------------------------------------------------------------------
ORACLE_MAX = 50_000


def reference(pods, recs, spec):
    """{(metric, label values): value} of one batch: the oracle per flow, the C port above
    ORACLE_MAX records (and above 10,000 pods, where the oracle's cache takes seconds)."""
    if len(recs) <= ORACLE_MAX and len(pods.endpoints) <= 10_000:
        return values_only(oracle_series(recs, pods, spec, False))
    return ref_series(pods, recs, spec, False)


def add_series(a: dict, b: dict) -> dict:
    out = dict(a)
    for k, v in b.items():
        out[k] = out.get(k, 0) + v
    return out


def check(g, want, what=""):
    got = values_only(g.snapshot())
    assert got == want, "%s: %s" % (what, diff_series(got, want))
    assert want, what


def see(be: Backend, g, name: Optional[str], what: str) -> str:
    """Reads the kernel's name (before the state is compared; asserted by `named` after it:
    a wrong state is the finding, the route explains it)."""
    got = g.kernel_name()
    print("%s: %s" % (what, got if be.gpu else "(host) expects " + str(name)))
    return got


def named(be: Backend, got: str, name: Optional[str]):
    if be.gpu and name is not None:
        assert got == name, (got, name)


def dense_len(g) -> int:
    """gpuagg_state().dense_len; read before the first submit (a state read folds what waits)."""
    return int(g.state().dense_len)


# ---- specs ----------------------------------------------------------------------------------
def _m(name, labels):
    return {"metric_name": name, "source_labels": list(labels)}


NP, POD = ("namespace", "podname"), ("podname",)
FWD = [_m("forward_count", NP), _m("forward_bytes", NP)]
FWD_DROP = W.LOCAL_FWD_DROP
TWO_FWD = [_m("forward_count", NP), _m("forward_bytes", ("workload",))]
FLAGS = [_m("tcp_flag_gauges", POD)]
FWD_FLAGS = [_m("forward_count", POD), _m("tcp_flag_gauges", POD)]
# four families, count and bytes of forward and drop (four groups)
FOUR = [_m("forward_count", POD), _m("forward_bytes", POD), _m("tcp_flag_gauges", POD), _m("drop_count", POD),
        _m("drop_bytes", POD), _m("tcp_retransmission_count", POD)]
SIX = [_m("forward_count", NP), _m("forward_bytes", ("workload",)), _m("drop_count", POD),
       _m("drop_bytes", ("namespace",)), _m("tcp_flag_gauges", POD), _m("tcp_retransmission_count", POD)]
KEYLESS_A = [_m("tcp_retransmission_count", ("service",)), _m("drop_count", ("workload",))]
KEYLESS_B = [_m("forward_count", ("service",)), _m("tcp_flag_gauges", POD)]
# keyless groups of nsub = 8: 16 bins each, behind a keyed forward group
KEYLESS_C = [_m("forward_count", POD), _m("tcp_flag_gauges", ("service",)), _m("drop_count", ("service",))]
DNS_ONLY = [_m("dns_request_count", POD)]
DNS_TWO = [_m("dns_request_count", POD), _m("dns_response_count", ("namespace",))]
EIGHT = SIX + DNS_TWO
FWD_FLAGS_RETRANS = FWD_FLAGS + [_m("tcp_retransmission_count", POD)]
DROP_ONLY = [_m("drop_count", POD), _m("drop_bytes", POD)]
SPECS = {"fwd": FWD, "fwd-drop": FWD_DROP, "two-fwd": TWO_FWD, "flags": FLAGS, "fwd-flags": FWD_FLAGS, "four": FOUR,
         "six": SIX, "keyless-a": KEYLESS_A, "keyless-b": KEYLESS_B, "keyless-c": KEYLESS_C,
         "dns-only": DNS_ONLY, "dns-two": DNS_TWO,
         "c5": W.C5_SPEC, "eight": EIGHT, "fwd-flags-retrans": FWD_FLAGS_RETRANS, "drop-only": DROP_ONLY}

MIX = dict(drop_frac=0.10, retrans_frac=0.05, udp_frac=0.2, other_proto_frac=0.05)
MIX_DNS = dict(MIX, dns_frac=0.2, n_queries=50)


def has_dns(spec) -> bool:
    return any(m["metric_name"].startswith("dns_") for m in spec)


@functools.lru_cache(maxsize=None)
def pods_of(n_pods: int):
    return W.make_pods(n_pods, seed=900)


@functools.lru_cache(maxsize=None)
def mixed(n_pods: int, n: int, dns: bool, seed: int = 0):
    """Seeded pods and the mixed records: 80 % of the addresses are pods, drops,
    retransmissions, UDP, other protocols, (dns) DNS queries and responses; the first rows are
    one record of each kind between pods, so the smallest batches update every family."""
    pods = pods_of(n_pods)
    recs = W.gen_records(n, pods, seed=910 + seed, **(MIX_DNS if dns else MIX))
    verdict, proto = (recs.meta >> 8) & 0xFF, recs.meta & 0xFF
    is_pod = np.isin(recs.src_ip, pods.ips[1:]) & np.isin(recs.dst_ip, pods.ips[1:]) & (recs.src_ip != recs.dst_ip)
    first = []
    for v in (W.V_FWD, W.V_DROP, W.V_RETRANS, W.V_FWD) + ((W.V_DNS,) if dns else ()):
        ok = np.flatnonzero((verdict == v) & is_pod & ((proto == W.PROTO_TCP) | (v == W.V_DNS)))
        first.append(int(next(i for i in ok if i not in first)))
    order = np.concatenate([first, np.setdiff1d(np.arange(n), first)])
    return pods, take(recs, order)


@functools.lru_cache(maxsize=None)
def mixed_reference(spec_id: str, n_pods: int, n: int, seed: int = 0, total: Optional[int] = None):
    """The reference of the first n of mixed(n_pods, total or n, ...), computed once."""
    spec = SPECS[spec_id]
    pods, recs = mixed(n_pods, total or n, has_dns(spec), seed)
    return reference(pods, take(recs, slice(0, n)), spec)


def run(be: Backend, spec, pods, parts, want, flags=0, name=None, unaligned=False, geo=None, what="", dns=None):
    """One engine, one unsynced submit per part, one snapshot; dense_len against the
    restated layout before the first submit, the kernel's name on the GPU.  dns: the batch
    whose DNS payloads a DNS plan interns (growth_inputs.slices leaves them behind)."""
    parts = list(parts)
    g = be.engine(pods, spec, flags, recs=(parts[0] if dns is None else dns) if has_dns(spec) else None)
    try:
        if geo is not None:
            assert dense_len(g) == geo.dense_len, (dense_len(g), geo.dense_len)
        keep = [be.submit(g, r, unaligned) for r in parts]
        got = see(be, g, name, what)
        check(g, want, what)
        del keep
        named(be, got, name)
        return got
    finally:
        g.close()


# ---- A. plan matrix -------------------------------------------------------------------------
# id -> (spec, pods, the kernel of the plain run as the launcher prints it, what the case is
# there for as (group index, in LDS) pairs).  The names are literals on purpose: kernel_name()
# has to reproduce them (on the CPU backend too), the GPU has to print them.
PLANS = {
    "fwd-lds": ("fwd", 300, "dense_lds_kernel<1, true, 9u, 2>", [(0, True)]),
    "fwd-drop-lds": ("fwd-drop", 300, "dense_lds_kernel<2, true, 169u, 2>", [(0, True), (1, True)]),
    # C2's production kernel at 3,000 pods: the drop group ends at 54,144 bins
    "fwd-lds-drop-spill": ("fwd-drop", 3000, "dense_lds_kernel<2, true, 41u, 2>", [(0, True), (1, False)]),
    "two-fwd": ("two-fwd", 300, "dense_lds_kernel<2, true, 0u, 2>", [(0, True), (1, True)]),
    # no LDS bins at all (L4 = 0, no stage_a)
    "flags-only-spilled": ("flags", 3000, "dense_lds_kernel<1, true, 0u, 2>", [(0, False)]),
    # almost every record enters the three-register SpillQ
    "fwd-lds-flags-spill": ("fwd-flags", 3000, "dense_lds_kernel<2, true, 0u, 2>", [(0, True), (1, False)]),
    "four-mixed-1500": ("four", 1500, "dense_lds_kernel<4, true, 0u, 2>", [(0, True), (1, True), (2, False), (3, False)]),
    "four-mixed-300": ("four", 300, "dense_lds_kernel<4, true, 0u, 2>", [(0, True), (1, True), (2, True), (3, True)]),
    "six-300": ("six", 300, "dense_lds_kernel<8, true, 0u, 2>", [(g, True) for g in range(6)]),
    "six-3000": ("six", 3000, "dense_lds_kernel<8, true, 0u, 2>", [(0, True), (1, True)] + [(g, False) for g in range(2, 6)]),
    # drop [workload] then the keyless retransmit group of 2 bins
    "keyless-a": ("keyless-a", 300, "dense_lds_kernel<2, true, 0u, 2>", [(0, True), (1, True)]),
    # the keyless forward group of 2 bins, then tcpflags at base 2: rows not 8-aligned
    "keyless-b": ("keyless-b", 300, "dense_lds_kernel<2, true, 0u, 2>", [(0, True), (1, True)]),
    # the keyless tcpflags and drop groups of 16 bins each behind forward [podname]
    "keyless-c": ("keyless-c", 300, "dense_lds_kernel<4, true, 0u, 2>", [(0, True), (1, True), (2, True)]),
    "dns-only": ("dns-only", 300, "dense_local_kernel<1, true, true, 0u>", []),
    "dns-two": ("dns-two", 300, "dense_local_kernel<2, true, true, 0u>", []),
    # tcpflags in LDS, so not kSigC5
    "c5-small": ("c5", 400, "dense_local_kernel<4, true, true, 0u>", [(0, True), (1, True)]),
    "c5-staged": ("c5", 3000, "dense_local_kernel<4, true, true, 25923u, true>", [(0, False), (1, False)]),
    "eight-300": ("eight", 300, "dense_local_kernel<8, true, true, 0u>", [(g, True) for g in range(6)]),
    "eight-3000": ("eight", 3000, "dense_local_kernel<8, true, true, 0u>", [(0, True), (1, True)] + [(g, False) for g in range(2, 6)]),
}
# the same plan through dense_local_kernel<NG, ., false, 0u>: GPUAGG_FLAG_NO_LDS_IP_TABLE
PLANS_TIER1 = [p for p, v in PLANS.items() if v[2].startswith("dense_lds")]
# (plan, flags, unaligned columns); the kVec = false form of every variant with flags 0
PLAN_RUNS = ([(p, f, False) for p in PLANS for f in (0, PER_BATCH)] +
             [(p, NO_LDS_IP | f, False) for p in PLANS_TIER1 for f in (0, PER_BATCH)] +
             [(p, 0, True) for p in PLANS] + [(p, NO_LDS_IP, True) for p in PLANS_TIER1])
# the LDS IP image's other two forms (kIp 0 / 1) through every tier-1 instantiation that
# iptable_cases.py (169u only) does not run with them: 9u, 41u and <1 / 2 / 4 / 8, ., 0u>
PLANS_KIP = ["fwd-lds", "fwd-lds-drop-spill", "flags-only-spilled", "two-fwd", "four-mixed-300", "six-300"]
PLAN_RUNS += [(p, f, u) for p in PLANS_KIP for f in (CUCKOO, ROW_RADIX) for u in (False, True)]
PLAN_SIZES = [10_000, 7, 20_004]
# four-mixed at 1,500 pods under tier 2: tcpflags ends at 27,648 > 20,288 bins, spilled there
TIER2_RESIDENCY = {"four-mixed-1500": [(0, True), (1, False), (2, False), (3, False)]}


def plan_id(run) -> str:
    return "%s-f%d%s" % (run[0], run[1], "-unaligned" if run[2] else "")


def plan_geometry(plan: str, flags: int) -> Geometry:
    spec_id, n_pods, name, resident = PLANS[plan]
    geo = geometry(SPECS[spec_id], pods_of(n_pods), flags)
    if flags & NO_LDS_IP:
        resident = TIER2_RESIDENCY.get(plan, resident)
    assert [(i, g.in_lds) for i, g in enumerate(geo.dense())] == resident, (plan, geo)
    assert geo.tier1 == (name.startswith("dense_lds") and not flags & NO_LDS_IP)
    return geo


def plan_matrix(be: Backend, plan: str, flags: int, unaligned: bool = False):
    spec_id, n_pods, literal, _ = PLANS[plan]
    spec = SPECS[spec_id]
    geo = plan_geometry(plan, flags)
    name = kernel_name(geo)
    if flags & (CUCKOO | ROW_RADIX):  # the literal but for its last argument
        assert geo.tier1 and name == literal[:-2] + ("0>" if flags & CUCKOO else "1>"), (name, literal)
    elif not flags & NO_LDS_IP:
        assert name == literal, (name, literal)
    else:
        assert name == "dense_local_kernel<%s, true, false, 0u>" % literal[len("dense_lds_kernel<")], name
    if plan == "dns-only":
        assert geo.dense_len == 0
    if plan == "keyless-a":
        assert [g.nbins for g in geo.dense()] == [16 * 320, 2]
    if plan == "keyless-b":
        assert [(g.base, g.nbins) for g in geo.dense()] == [(0, 2), (2, 16 * 320)] and geo.dense()[1].base % 8
    if plan == "keyless-c":
        assert [(g.fam, g.base, g.nbins) for g in geo.dense()] == [(FAM_FWD, 0, 2 * 320), (FAM_TCPFLAGS, 640, 16),
                                                                   (FAM_DROP, 656, 16)]
    n = sum(PLAN_SIZES)
    pods, recs = mixed(n_pods, n, has_dns(spec))
    # uniform input: every (workgroup, window) list stays short -- the fold's wave-per-list walk
    assert launch_chunk(n, be.cus) * 16 < FOLD_WAVE_PER_LIST
    if unaligned:
        name = kernel_name(geo, vec=False)
        assert name == kernel_name(geo).replace(", true,", ", false,", 1)
    run(be, spec, pods, slices(recs, PLAN_SIZES), mixed_reference(spec_id, n_pods, n), flags, name, unaligned=unaligned,
        geo=geo, what=plan_id((plan, flags, unaligned)), dns=recs)


# ---- B. launch shape ------------------------------------------------------------------------
SHAPE_PLANS = ["fwd-lds-drop-spill", "four-mixed-1500", "c5-staged"]
SHAPE_N = ["1", "3", "4", "5", "63", "64", "65", "cu-1", "cu", "cu+1", "4cu+3", "4096cu+1"]
SHAPE_RUNS = [(p, n, u, f) for p in SHAPE_PLANS for n in SHAPE_N for u in (False, True) for f in (0, PER_BATCH)]


def shape_n(be: Backend, which: str) -> int:
    cu = be.cus
    return {"cu-1": cu - 1, "cu": cu, "cu+1": cu + 1, "4cu+3": 4 * cu + 3, "4096cu+1": 4096 * cu + 1}.get(which) or int(which)


def launch_shape(be: Backend, plan: str, which: str, unaligned, flags: int):
    """n below the number of workgroups (chunk = 4: most workgroups start at or past n), ragged
    tails (n % 4: the vector body and the scalar tail), one record more than a full 4,096 per
    workgroup; unaligned columns take the kVec = false kernel -- one misaligned column is
    enough."""
    spec_id, n_pods, _, _ = PLANS[plan]
    spec = SPECS[spec_id]
    n, total = shape_n(be, which), 4096 * be.cus + 1
    pods, recs = mixed(n_pods, total, has_dns(spec), 1)
    name = kernel_name(plan_geometry(plan, flags), vec=not unaligned)
    assert ("false" if unaligned else "true") in name.split(",")[1]
    run(be, spec, pods, [take(recs, slice(0, n))], mixed_reference(spec_id, n_pods, n, 1, total), flags, name,
        unaligned=unaligned, what="%s n=%d unaligned=%s f%d" % (plan, n, unaligned, flags))


# ---- C. byte-field edges ----------------------------------------------------------------------
# each bin's two sides through these byte counts: around the spill entry's 2^18, tier 1's
# 20-bit LDS field, tier 2's 2^24 (kLdsByteLimit), the C2 queue's kQBytes = 2^29 - 1, and 2^32
EDGE_BYTES = np.array([0, (1 << 18) - 1, 1 << 18, 1 << 19, (1 << 20) - 1, 1 << 20, (1 << 24) - 1, 1 << 24,
                       (1 << 29) - 1, 1 << 29, (1 << 32) - 1, 1, 1500, (1 << 20) + 1, 1 << 31, (1 << 31) + 5], np.uint32)
EDGE_REPEAT = 1 << 14  # 64 distinct records x 2^14 = 2^20 records
EDGE_REASON = 3
# id -> (plan, flags, the bins the case is about)
EDGE_CASES = {
    "t1-lds": ("fwd-drop-lds", 0),               # forward and drop bins, u32 count:12 | bytes:20
    "t2-lds": ("fwd-drop-lds", NO_LDS_IP),       # the same bins, u64 count:20 | bytes:44
    "c2-queue": ("fwd-lds-drop-spill", 0),       # spilled drop bin, two-register queue
    "generic-queue": ("four-mixed-1500", 0),     # spilled drop bin, three-register SpillQ
    "t2-spill": ("fwd-lds-drop-spill", NO_LDS_IP),
}
EDGE_RUNS = [(c, f) for c in EDGE_CASES for f in (0, PER_BATCH)]


@functools.lru_cache(maxsize=None)
def edge_records(n_pods: int):
    """(pods, the 64 distinct records): pods 5 -> 7 and 7 -> 5, forwarded and dropped with
    EDGE_REASON, each at every EDGE_BYTES value."""
    pods = pods_of(n_pods)
    a, b = (np.uint32(pods.endpoints[i].ips[0]) for i in (5, 7))
    src, dst, nbytes, meta = [], [], [], []
    for s, d in ((a, b), (b, a)):
        for verdict, tdir, reason in ((W.V_FWD, 2, 0), (W.V_DROP, 1, EDGE_REASON)):
            for x in EDGE_BYTES:
                src.append(s), dst.append(d), nbytes.append(x)
                meta.append(W.pack_meta(W.PROTO_TCP, verdict, tdir, reason, W.ACK if verdict == W.V_FWD else 0))
    k, u = len(src), np.uint32
    return pods, W.Records(np.array(src, u), np.array(dst, u), np.array(nbytes, u), np.array(meta, u),
                           np.full(k, 40000 | (443 << 16), u), np.zeros(k, u))


def byte_edges(be: Backend, case: str, flags: int):
    """Linearity: the reference of the 64 distinct records times EDGE_REPEAT.  Each distinct
    record fills whole workgroup chunks, so on tier 1 a bin takes 4,096 adds in one workgroup:
    the 12-bit count wraps and the 20-bit bytes carry (asserted from the input)."""
    plan, plan_flags = EDGE_CASES[case]
    spec_id, n_pods, _, _ = PLANS[plan]
    spec = SPECS[spec_id]
    flags |= plan_flags
    geo = plan_geometry(plan, flags)
    pods, distinct = edge_records(n_pods)
    recs = take(distinct, np.repeat(np.arange(len(distinct)), EDGE_REPEAT))
    n = len(recs)
    assert 200_000 <= n <= 1 << 20
    chunk = launch_chunk(n, be.cus)
    # per workgroup: the adds and the LDS-field bytes of the busiest bin (a run of one record)
    wg = np.arange(n) // chunk
    run_len = np.bincount(wg * len(distinct) + np.repeat(np.arange(len(distinct)), EDGE_REPEAT)).max()
    if case == "t1-lds":  # (needs chunk >= 4,096: at most 256 workgroups)
        in_field = EDGE_BYTES[EDGE_BYTES < L4_BYTE_LIMIT].astype(np.int64)
        assert run_len >= L4_COUNT_LIMIT and (run_len * in_field >= L4_BYTE_LIMIT).sum() >= 4
    drop = next(g for g in geo.dense() if g.fam == FAM_DROP)
    assert drop.in_lds == (case in ("t1-lds", "t2-lds"))
    if not drop.in_lds:  # the entries' byte field on both sides of its limit, and the queue's
        assert geo.nwin and (EDGE_BYTES == ENTRY_BYTES_LIMIT - 1).any() and (EDGE_BYTES == ENTRY_BYTES_LIMIT).any()
        assert (EDGE_BYTES == Q_BYTES).any() and (EDGE_BYTES == Q_BYTES + 1).any()
    want = scale_series(reference(pods, distinct, spec), EDGE_REPEAT)
    run(be, spec, pods, [recs], want, flags, kernel_name(geo), geo=geo, what="%s f%d" % (case, flags))


# ---- D. spill-fold geometry -------------------------------------------------------------------
def bin_of(g: Group, slot: int, side: int, sub: int = 0) -> int:
    """l4_records / dense_local_kernel: side 0 ingress (the destination pod), 1 egress."""
    return g.base + ((slot if g.keyed else 0) * 2 + side) * g.nsub + sub


def window_of(geo: Geometry, b: int) -> int:
    return (b - geo.L) >> FOLD_WINDOW_SHIFT


ONE_WINDOW = {"tier1": (2048, 0), "tier2": (1088, NO_LDS_IP)}


def one_window(be: Backend, tier: str, flags: int):
    """forward + tcpflags fill the LDS prefix, the retransmit group behind them is the whole
    spilled remainder: one window (nwin = 1, one fold workgroup per partition)."""
    n_pods, tier_flags = ONE_WINDOW[tier]
    flags |= tier_flags
    pods = pods_of(n_pods)
    geo = geometry(FWD_FLAGS_RETRANS, pods, flags)
    assert [g.in_lds for g in geo.dense()] == [True, True, False] and geo.tier1 == (tier == "tier1")
    assert 0 < geo.dense_len - geo.L <= FOLD_WINDOW_BINS and geo.nwin == 1
    pods, recs = mixed(n_pods, 30_011, False, 2)
    run(be, FWD_FLAGS_RETRANS, pods, slices(recs, PLAN_SIZES), mixed_reference("fwd-flags-retrans", n_pods, 30_011, 2),
        flags, kernel_name(geo), geo=geo, what="one-window %s f%d" % (tier, flags))


PARTIAL_PODS = 2624  # key_cap 2,624: 41,984 bins of drops, five windows and 1,024 bins


@functools.lru_cache(maxsize=None)
def partial_window_inputs():
    pods, recs = mixed(PARTIAL_PODS, 30_000, False, 3)
    geo = geometry(DROP_ONLY, pods, 0)
    g = geo.dense()[0]
    ext = np.uint32(W.ip_le(100, 64, 0, 1))
    # (slot, side, reason): the last bin of the state, the first and the last bin of window 3
    placed = [(PARTIAL_PODS - 1, 1, 7), (3 * FOLD_WINDOW_BINS // 16, 0, 0), (4 * FOLD_WINDOW_BINS // 16 - 1, 1, 7)]
    assert [bin_of(g, *p) for p in placed] == [geo.dense_len - 1, 3 * FOLD_WINDOW_BINS, 4 * FOLD_WINDOW_BINS - 1]
    k, u = len(placed), np.uint32
    ip = [u(pods.endpoints[s].ips[0]) for s, _, _ in placed]
    extra = W.Records(np.array([i if side else ext for i, (_, side, _) in zip(ip, placed)], u),
                      np.array([ext if side else i for i, (_, side, _) in zip(ip, placed)], u),
                      np.array([700, 1 << 18, (1 << 18) - 1], u),
                      np.array([W.pack_meta(W.PROTO_TCP, W.V_DROP, 1, r) for _, _, r in placed], u),
                      np.full(k, 40000 | (80 << 16), u), np.zeros(k, u))
    both = W.Records(*[np.concatenate([getattr(extra, c), getattr(recs, c)])
                       for c in ("src_ip", "dst_ip", "bytes", "meta", "ports", "dns_id")])
    return pods, both, placed, reference(pods, both, DROP_ONLY)


def partial_window(be: Backend, flags: int):
    """No group fits (L = 0) and the last window is partial: hi = min(lo + W, dense_len) in
    spill_window_kernel, stage_reduce_b's guard.  Three placed drops update the last bin of the
    state and the first and last bin of a middle window."""
    pods, recs, placed, want = partial_window_inputs()
    geo = geometry(DROP_ONLY, pods, flags)
    assert geo.L == 0 and geo.dense_len % FOLD_WINDOW_BINS != 0 and geo.nwin == 6
    for slot, _, _ in placed:  # the series of the placed bins are in the reference
        assert any(k[1][-1] == pods.endpoints[slot].name for k in want), pods.endpoints[slot].name
    run(be, DROP_ONLY, pods, slices(recs, [3, 10_000, 20_000]), want, flags, kernel_name(geo), geo=geo,
        what="partial-window f%d" % flags)


# the "six" spec has 54 bins per key: key_cap 38,784 is 256 windows, 38,848 is 257 (no lists:
# every spilled update a global atomic).  The first group (77k+ bins) fits no prefix: L = 0.
BOUNDARY = {"256": 38_784, "257": 38_785}


@functools.lru_cache(maxsize=None)
def boundary_inputs(n_pods: int):
    pods, recs = mixed(n_pods, 50_000, False, 4)
    return pods, recs, ref_series(pods, recs, SIX, False)


def window_boundary(be: Backend, which: str, flags: int):
    n_pods = BOUNDARY[which]
    pods, recs, want = boundary_inputs(n_pods)
    geo = geometry(SIX, pods, flags)
    assert geo.L == 0 and not geo.tier1  # (38k pods: no LDS image of their addresses fits)
    assert geo.dense_len == 54 * key_cap_for(n_pods) and geo.windows == int(which)
    assert geo.nwin == (256 if which == "256" else 0)
    run(be, SIX, pods, slices(recs, [20_000, 9, 29_991]), want, flags, kernel_name(geo), geo=geo,
        what="boundary %s f%d" % (which, flags))


NO_RINGS_PODS = 120_000


@functools.lru_cache(maxsize=None)
def no_rings_inputs():
    pods = pods_of(NO_RINGS_PODS)
    recs = W.gen_records(50_000, pods, seed=925, retrans_frac=0.05, dns_frac=0.3, n_queries=500, drop_frac=0.0)
    return pods, recs, ref_series(pods, recs, W.C5_SPEC, False)


def c5_no_rings(be: Backend, flags: int, unaligned: bool = False):
    """C5 at 120,000 pods: 2,160,000 bins, more than 256 windows -- kSigC5 without lists or
    rings, every tcpflags / retransmit update a global atomic."""
    pods, recs, want = no_rings_inputs()
    geo = geometry(W.C5_SPEC, pods, flags)
    assert geo.windows > MAX_SPILL_WINDOWS and geo.nwin == 0 and geo.sig == SIG_C5
    name = kernel_name(geo, vec=not unaligned)
    assert name == "dense_local_kernel<4, %s, true, 25923u>" % ("false" if unaligned else "true")
    run(be, W.C5_SPEC, pods, slices(recs, 2), want, flags, name, unaligned=unaligned, geo=geo,
        what="c5-no-rings f%d%s" % (flags, " unaligned" if unaligned else ""), dns=recs)


def hot_pair(pods, geo: Geometry, fam: int):
    """Two pods whose bins of the family's group share a window; (source, destination)."""
    g = next(x for x in geo.dense() if x.fam == fam)
    a, b = 5, 7
    bins = [bin_of(g, a, 1, EDGE_REASON if fam == FAM_DROP else 0), bin_of(g, b, 0, EDGE_REASON if fam == FAM_DROP else 0)]
    assert not g.in_lds and window_of(geo, bins[0]) == window_of(geo, bins[1])
    return np.uint32(pods.endpoints[a].ips[0]), np.uint32(pods.endpoints[b].ips[0]), window_of(geo, bins[0])


def hot_drops(pods, geo: Geometry, n: int, distinct_bytes=(64, 1500, (1 << 18) - 1, 1 << 18)):
    """(the distinct records, the batch of n): every record a drop with EDGE_REASON from pod 5 to
    pod 7, both bins in one window."""
    a, b, _ = hot_pair(pods, geo, FAM_DROP)
    k, u = len(distinct_bytes), np.uint32
    assert n % k == 0
    distinct = W.Records(np.full(k, a, u), np.full(k, b, u), np.array(distinct_bytes, u),
                         np.full(k, W.pack_meta(W.PROTO_TCP, W.V_DROP, 1, EDGE_REASON), u),
                         np.full(k, 40000 | (443 << 16), u), np.zeros(k, u))
    return distinct, take(distinct, np.tile(np.arange(k), n // k))


HOT = {"c2": ("fwd-lds-drop-spill", 0), "generic": ("four-mixed-1500", 0), "tier2": ("fwd-lds-drop-spill", NO_LDS_IP)}
HOT_N = 1 << 20


def hot_bin_per_batch(be: Backend, variant: str):
    """FLAG_FOLD_PER_BATCH, 2^20 drops on one pod pair: each workgroup's 2 * chunk entries for
    one window overflow its list (spill_cap = 2 * chunk / nwin + 4096) into the global
    fallback, and the fold walks the hot window's long lists workgroup-wide."""
    plan, flags = HOT[variant]
    flags |= PER_BATCH
    spec_id, n_pods, _, _ = PLANS[plan]
    spec, pods = SPECS[spec_id], pods_of(n_pods)
    geo = plan_geometry(plan, flags)
    distinct, recs = hot_drops(pods, geo, HOT_N)
    chunk = launch_chunk(HOT_N, be.cus)
    cap = spill_cap(geo, chunk, True)
    nparts, lists_here = fold_partitions(geo, be.cus)
    assert 2 * chunk > cap, "the hot lists do not overflow"
    assert cap >= FOLD_WAVE_PER_LIST  # full lists: total >= lists_here * 2048, the workgroup-wide walk
    want = scale_series(reference(pods, distinct, spec), HOT_N // len(distinct))
    run(be, spec, pods, [recs], want, flags, kernel_name(geo), geo=geo, what="hot per-batch %s" % variant)


HOT_DEFER_N, HOT_DEFER_SUBMITS = 1 << 18, 40


def hot_bin_deferred(be: Backend, variant: str, fold_flags: int = 0):
    """The same batch of 2^18 records (half drops, half forwarded) 40 times, unsynced, then one
    snapshot: the lists fill across launches (accum, spill_ctr0) and overflow, tier 1 continues
    from its staged copy (stage_accum: 40 x 1,024 adds per workgroup wrap the 12-bit counts of
    the copy).  With FLAG_FOLD_PER_BATCH the same 40 launches each fold and reduce alone."""
    plan, flags = HOT[variant]
    flags |= fold_flags
    spec_id, n_pods, _, _ = PLANS[plan]
    spec, pods = SPECS[spec_id], pods_of(n_pods)
    geo = plan_geometry(plan, flags)
    dropped, _ = hot_drops(pods, geo, 4)
    fwd = W.Records(dropped.src_ip, dropped.dst_ip, dropped.bytes,
                    np.full(4, W.pack_meta(W.PROTO_TCP, W.V_FWD, 2, 0, W.ACK), np.uint32), dropped.ports, dropped.dns_id)
    distinct = W.Records(*[np.concatenate([getattr(dropped, c), getattr(fwd, c)])
                           for c in ("src_ip", "dst_ip", "bytes", "meta", "ports", "dns_id")])
    recs = take(distinct, np.tile(np.arange(8), HOT_DEFER_N // 8))
    chunk = launch_chunk(HOT_DEFER_N, be.cus)
    assert chunk <= SMALL_LAUNCH_CHUNK and HOT_DEFER_SUBMITS <= DEFER_LAUNCHES
    if not fold_flags:
        assert HOT_DEFER_SUBMITS * chunk > spill_cap(geo, chunk, False), "the accumulated lists do not overflow"
    assert HOT_DEFER_SUBMITS * chunk // 2 >= L4_COUNT_LIMIT, "the staged 12-bit counts do not wrap (%d workgroups)" % be.cus
    want = scale_series(reference(pods, distinct, spec), HOT_DEFER_SUBMITS * HOT_DEFER_N // 8)
    g = be.engine(pods, spec, flags)
    try:
        assert dense_len(g) == geo.dense_len
        keep = be.submit(g, recs)
        for _ in range(HOT_DEFER_SUBMITS - 1):
            if be.gpu:
                from retina_amd import GpuAgg
                g.submit_device(GpuAgg.device_columns(*keep), len(recs))
            else:
                g.submit_numpy(recs)
        got = see(be, g, kernel_name(geo), "hot deferred %s f%d" % (variant, flags))
        check(g, want, "hot deferred %s f%d" % (variant, flags))
        del keep
        named(be, got, kernel_name(geo))
    finally:
        g.close()


EXACT_FOLD_N = 1 << 21


def exact_fold(be: Backend):
    """The fold's exact add: the "six" spec at 256 windows has two fold partitions of 128
    lists.  One deferred launch of 2^21 drops from one pod to an address that is no pod's puts
    a workgroup's 8,192 records into one bin of the [podname] group (and one of the
    [namespace] group): each list of those windows is exactly full at its capacity of 8,192,
    so a partition reads 2^20 entries (fast = total < 2^20 is false) and adds all of them to
    one bin -- the 20-bit count of the fold window wraps on the last one, which only the
    carrying add books.  Every other window is empty (the fast add)."""
    n_pods = BOUNDARY["256"]
    pods = pods_of(n_pods)
    geo = geometry(SIX, pods, 0)
    k, u = 4, np.uint32
    ext = W.ip_le(100, 64, 0, 1)
    assert ext not in set(pods.ips.tolist())
    distinct = W.Records(np.full(k, pods.endpoints[5].ips[0], u), np.full(k, ext, u),
                         np.array([64, 1500, (1 << 18) - 1, 1 << 18], u),
                         np.full(k, W.pack_meta(W.PROTO_TCP, W.V_DROP, 1, EDGE_REASON), u),
                         np.full(k, 40000 | (443 << 16), u), np.zeros(k, u))
    recs = take(distinct, np.tile(np.arange(k), EXACT_FOLD_N // k))
    chunk = launch_chunk(EXACT_FOLD_N, be.cus)
    cap = spill_cap(geo, chunk, False)
    nparts, lists_here = fold_partitions(geo, be.cus)
    # one entry per record and group: every list full, none past its capacity.  The sizes are
    # those of 256 workgroups; on another device the case has to be re-sized, not weakened
    assert be.cus == 256, "exact_fold is sized for 256 workgroups, the device has %d" % be.cus
    assert (nparts, lists_here, cap, chunk) == (2, 128, 8192, 8192) and chunk <= SMALL_LAUNCH_CHUNK
    assert cap * lists_here == FOLD_EXACT_ENTRIES == 1 << (64 - 44)  # the window's count field: 20 bits
    want = scale_series(ref_series(pods, distinct, SIX, False), EXACT_FOLD_N // k)
    run(be, SIX, pods, [recs], want, 0, kernel_name(geo), geo=geo, what="exact-fold")


RING_N = 300_000


@functools.lru_cache(maxsize=None)
def ring_inputs(kind: str):
    """hot: every record a forwarded TCP packet between pods 5 and 7 -- all flag bits, then SYN
    alone and ACK | URG, so all seven flag labels count; uniform: the same three packets
    spread over all pods."""
    pods = pods_of(3000)
    u = np.uint32
    flags3 = np.array([0x3F, W.SYN, W.ACK | W.URG], u)
    if kind == "hot":
        k = 3
        distinct = W.Records(np.full(k, pods.endpoints[5].ips[0], u), np.full(k, pods.endpoints[7].ips[0], u),
                             np.array([64, 1500, 9000], u), W.pack_meta(W.PROTO_TCP, W.V_FWD, 2, 0, flags3).astype(u),
                             np.full(k, 40000 | (443 << 16), u), np.zeros(k, u))
        return pods, take(distinct, np.tile(np.arange(k), RING_N // k)), scale_series(
            reference(pods, distinct, W.C5_SPEC), RING_N // k)
    rng = np.random.default_rng(926)
    recs = W.Records(pods.ips[rng.integers(1, len(pods.ips), RING_N)].astype(u),
                     pods.ips[rng.integers(1, len(pods.ips), RING_N)].astype(u), np.full(RING_N, 64, u),
                     W.pack_meta(W.PROTO_TCP, W.V_FWD, 2, 0, flags3[rng.integers(0, 3, RING_N)]).astype(u),
                     np.full(RING_N, 40000 | (443 << 16), u), np.zeros(RING_N, u))
    return pods, recs, ref_series(pods, recs, W.C5_SPEC, False)


def staged_rings(be: Backend, kind: str, flags: int):
    """c5-staged with the LDS rings: hot -- a workgroup's ~1,172 records put two row-mask
    entries each into one window's 128-entry ring between two flushes (4 steps x 4,096
    records): the ring overflows into the list (p >= kSpillRing).  The list itself does not
    fill at this size (2 * chunk entries against 2 * chunk / nwin + 4096, asserted): that is
    `ring_full`'s subject."""
    pods, recs, want = ring_inputs(kind)
    geo = plan_geometry("c5-staged", flags)
    assert geo.dense()[0].base % 8 == 0 and (geo.dense()[0].base - geo.L) % 8 == 0  # row masks
    chunk = launch_chunk(RING_N, be.cus)
    if kind == "hot":
        assert SPILL_RING < 2 * chunk <= spill_cap(geo, chunk, True)
        _, _, w = hot_pair(pods, geo, FAM_TCPFLAGS)
        assert w == 0
    run(be, W.C5_SPEC, pods, [recs], want, flags, kernel_name(geo), geo=geo, what="rings %s f%d" % (kind, flags))


# (records a submit, submits): one per-batch launch whose lists are too short for it; 40
# deferred launches into lists sized for 64 launches of uniform records
RING_FULL = {PER_BATCH: (1 << 21, 1), 0: (1 << 17, 40)}


@functools.lru_cache(maxsize=None)
def ring_full_distinct():
    """Eight records from pod 5 to pod 7: four forwarded TCP packets (all flag bits, SYN, ACK |
    URG, FIN | PSH: a row-mask entry for each side's tcpflags row) and four retransmissions (a
    plain entry for each side's bin)."""
    pods = pods_of(3000)
    u, k = np.uint32, 8
    meta = np.concatenate([W.pack_meta(W.PROTO_TCP, W.V_FWD, 2, 0, np.array([0x3F, W.SYN, W.ACK | W.URG, W.FIN | W.PSH], u)),
                           np.full(4, W.pack_meta(W.PROTO_TCP, W.V_RETRANS, 2, 0, W.ACK), u)]).astype(u)
    distinct = W.Records(np.full(k, pods.endpoints[5].ips[0], u), np.full(k, pods.endpoints[7].ips[0], u),
                         np.array([64, 1500, 9000, 40] * 2, u), meta, np.full(k, 40000 | (443 << 16), u), np.zeros(k, u))
    return pods, distinct, reference(pods, distinct, W.C5_SPEC)


def ring_full(be: Backend, flags: int):
    """c5-staged with full lists: every workgroup's records update one tcpflags window (two
    row-mask entries a forwarded packet) and one retransmit window (two plain entries a
    retransmission), more often than a list has room (asserted from the input for every
    workgroup and both windows) -- per batch in one launch of 2^21 records, deferred across 40
    unsynced launches of 2^17 (accum: ds.ctr continues from spill_count).  What no longer fits
    leaves through entry_global, from the ring's flush() and from spill_e's direct store, in
    its row-mask and its plain branch."""
    assert flags in RING_FULL
    n, submits = RING_FULL[flags]
    pods, distinct, one = ring_full_distinct()
    k = len(distinct)
    geo = plan_geometry("c5-staged", flags)
    assert geo.dense()[0].base % 8 == 0 and (geo.dense()[0].base - geo.L) % 8 == 0  # row masks
    idx = np.tile(np.arange(k), n // k)
    recs = take(distinct, idx)
    chunk = launch_chunk(n, be.cus)
    cap = spill_cap(geo, chunk, bool(flags & PER_BATCH))
    assert submits <= DEFER_LAUNCHES and (submits == 1 or chunk <= SMALL_LAUNCH_CHUNK)
    wg = np.arange(n) // chunk
    windows = []
    for fam, hit in ((FAM_TCPFLAGS, idx < 4), (FAM_RETRANS, idx >= 4)):
        _, _, w = hot_pair(pods, geo, fam)
        windows.append(w)
        entries = 2 * submits * np.bincount(wg[hit], minlength=int(wg[-1]) + 1)
        print("ring-full f%d: window %d takes %d..%d entries a workgroup, spill_cap %d" % (
            flags, w, entries.min(), entries.max(), cap))
        assert entries.min() > cap, "a list of window %d does not fill: %d <= %d" % (w, entries.min(), cap)
    assert windows[0] != windows[1] and 2 * chunk > SPILL_RING
    want = scale_series(one, submits * (n // k))
    name = kernel_name(geo)
    g = be.engine(pods, W.C5_SPEC, flags, recs=recs)
    try:
        assert dense_len(g) == geo.dense_len
        keep = be.submit(g, recs)
        for _ in range(submits - 1):
            if be.gpu:
                from retina_amd import GpuAgg
                g.submit_device(GpuAgg.device_columns(*keep), len(recs))
            else:
                g.submit_numpy(recs)
        got = see(be, g, name, "ring-full f%d" % flags)
        check(g, want, "ring-full f%d" % flags)
        del keep
        named(be, got, name)
    finally:
        g.close()


# ---- E. state changes under pending lists ---------------------------------------------------
STATE_PLANS = ["fwd-lds-drop-spill", "c5-staged"]
STATE_N = 40_000


@functools.lru_cache(maxsize=None)
def state_inputs(plan: str):
    """(pods, the pods with 100 more, two batches): the second batch drawn over the larger set."""
    spec_id, n_pods, _, _ = PLANS[plan]
    dns = has_dns(SPECS[spec_id])
    pods = pods_of(n_pods)
    big = W.make_pods(n_pods + 100, seed=900)
    more = W.Pods(pods.endpoints + big.endpoints[n_pods:], np.concatenate([pods.ips, big.ips[big.ip_owner >= n_pods]]),
                  np.concatenate([pods.ip_owner, big.ip_owner[big.ip_owner >= n_pods]]))
    assert len(set(more.ips.tolist())) == len(more.ips)
    recs = W.gen_records(2 * STATE_N, more, seed=930, **(MIX_DNS if dns else MIX))
    return pods, more, take(recs, slice(0, STATE_N)), take(recs, slice(STATE_N, 2 * STATE_N))


def _state_engine(be, plan, pods, first):
    spec_id = PLANS[plan][0]
    geo = plan_geometry(plan, 0)
    g = be.engine(pods, SPECS[spec_id], 0, recs=first if has_dns(SPECS[spec_id]) else None,
                  max_slots=len(pods.endpoints) + 256, max_ips=len(pods.ips) + 256)
    assert dense_len(g) == geo.dense_len
    return g, SPECS[spec_id], kernel_name(geo)


def state_reset(be: Backend, plan: str):
    """submit -> reset() -> submit: the waiting lists and staged copies are dropped."""
    pods, _, one, two = state_inputs(plan)
    g, spec, name = _state_engine(be, plan, pods, one)
    try:
        keep = [be.submit(g, one)]
        got = see(be, g, name, "reset %s" % plan)
        g.reset()
        keep.append(be.submit(g, two))
        check(g, reference(pods, two, spec), "reset %s" % plan)
        named(be, got, name)
        assert g.kernel_name() == got
    finally:
        g.close()


def state_relayout(be: Backend, plan: str):
    """submit -> 100 more pods (the dense re-layout with keep folds what waits, key_cap grows
    by 128) -> submit: the first batch under the old cache plus the second under the new."""
    pods, more, one, two = state_inputs(plan)
    g, spec, name = _state_engine(be, plan, pods, one)
    try:
        keep = [be.submit(g, one)]
        got = see(be, g, name, "relayout %s" % plan)
        g.load_endpoints(more.endpoints[len(pods.endpoints):])
        keep.append(be.submit(g, two))
        want = add_series(reference(pods, one, spec), reference(more, two, spec))
        check(g, want, "relayout %s" % plan)
        assert dense_len(g) == geometry(spec, more, 0).dense_len > geometry(spec, pods, 0).dense_len
        named(be, got, name)
    finally:
        g.close()


def state_reconcile(be: Backend, plan: str):
    """submit -> reconcile to another spec (a new layout, the state cleared, the waiting lists
    dropped) -> submit: the new spec over the second batch only."""
    pods, _, one, two = state_inputs(plan)
    g, spec, name = _state_engine(be, plan, pods, one)
    other = FOUR if plan == "c5-staged" else SIX
    try:
        keep = [be.submit(g, one)]
        got = see(be, g, name, "reconcile %s" % plan)
        g.reconcile(other)
        keep.append(be.submit(g, two))
        name2 = see(be, g, kernel_name(geometry(other, pods, 0)), "reconcile %s, after" % plan)
        check(g, reference(pods, two, other), "reconcile %s" % plan)
        named(be, got, name)
        named(be, name2, kernel_name(geometry(other, pods, 0)))
    finally:
        g.close()


def state_double(be: Backend, plan: str):
    """submit -> snapshot -> the same submit -> snapshot: every series doubles."""
    pods, _, one, _ = state_inputs(plan)
    g, spec, name = _state_engine(be, plan, pods, one)
    try:
        want = reference(pods, one, spec)
        keep = [be.submit(g, one)]
        check(g, want, "double %s, first" % plan)
        keep.append(be.submit(g, one))
        got = see(be, g, name, "double %s" % plan)
        check(g, scale_series(want, 2), "double %s, second" % plan)
        named(be, got, name)
    finally:
        g.close()
