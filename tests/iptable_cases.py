"""Inputs of the IP -> pod lookup tests, written once and run on both backends:
test_iptable_cpu.py (GPUAGG_FLAG_CPU_BACKEND, host-fed: inputs and oracle agree, and the
host radix mirror at the prefix-count boundaries) and test_gpu_iptable.py (gfx950: every
device form of the lookup under every kernel that reaches it, the kernel asserted by name).

Pod sets whose IPs fall in a chosen number of /16 prefixes (the thresholds of the forms:
kIprMaxPfx = 4, kRadixSmall = 8, kRadixMaxBlocks = 64) in layouts that stress the dense
radix image (holes, runs touching third octet 0 and 255, runs too long for the image);
records whose addresses almost match a pod; and the table of cases with the kernel name
each one must run, written out from launch_aggregate (gpuagg_kernels.hip) -- not computed."""

from __future__ import annotations

import functools
from typing import NamedTuple, Tuple, Union

import numpy as np

from retina_amd import _abi
from retina_amd import workloads as W

from .helpers import intern_dns, oracle_series, to_device

CPU = _abi.FLAG_CPU_BACKEND
NO_LDS, NO_RADIX = _abi.FLAG_NO_LDS_IP_TABLE, 4  # GPUAGG_FLAG_NO_RADIX_IP_TABLE
CUCKOO, ROW_RADIX = _abi.FLAG_LDS_CUCKOO, _abi.FLAG_ROW_RADIX
NO_WIDE_LISTS = _abi.FLAG_NO_WIDE_LISTS

PREFIX_COUNTS = (1, 4, 5, 8, 9, 64, 65)
LAYOUTS = ("run", "holes", "edges", "too-wide")
# last octets of the "edges" layout: the ends of a /24 first
_EDGE_LAST = [0, 255] + [16 * m + 5 for m in range(1, 15)]


def _addr(layout: str, npfx: int, i: int) -> int:
    j, k = i % npfx, i // npfx
    second = 3 * j + 1
    if layout == "run":
        return W.ip_le(10, second, 7 + (k >> 4), 16 * (k & 15) + 5)
    if layout == "holes":  # third octets 3, 9 and 200 only: the dense image fills the gaps with empty blocks
        return W.ip_le(10, second, (3, 9, 200)[(k >> 4) % 3], 16 * (k & 15) + 5 + k // 48)
    if layout == "edges":  # prefix 0: a run from third octet 0 up; prefix 1: a run down from 255
        return W.ip_le(10, second, (k >> 4) if j == 0 else 255 - (k >> 4), _EDGE_LAST[k & 15])
    if layout == "too-wide":  # every 16th third octet: runs of 241 /24s, 16 of them populated
        return W.ip_le(10, second, 16 * (k & 15) + j, 16 * ((k >> 4) & 15) + 5)
    raise ValueError(layout)


@functools.lru_cache(maxsize=None)
def pods_in_prefixes(npfx: int, per: int = 40, seed: int = 0, layout: str = "run") -> W.Pods:
    """npfx * per single-IP pods in npfx /16 prefixes (10.1, 10.4, 10.7, ...): make_pods with
    the IPs rewritten, so pod 0 stays the apiserver pseudo pod (left out of the tier-1
    image, kept in the all-pods one; in local context its IP is no endpoint).
    "too-wide": iprd_build refuses (npfx * 241 + 1 blocks of 512 B > 112 KiB) while
    ipr_build accepts (16 * npfx blocks); at most 4 prefixes.  "edges": 2 prefixes.
    "holes": 198 blocks a prefix, so the dense image takes one prefix only."""
    assert layout in LAYOUTS and npfx >= 1
    assert layout != "edges" or npfx == 2
    assert layout != "too-wide" or (npfx <= 4 and per <= 256)
    assert layout != "holes" or per <= 48 * 11
    base = W.make_pods(npfx * per, seed=seed, secondary_frac=0.0)
    ips = np.array([_addr(layout, npfx, i) for i in range(npfx * per)], np.uint32)
    assert len(np.unique(ips)) == len(ips) and len(np.unique(ips & np.uint32(0xFFFF))) == npfx
    assert base.endpoints[0].name == W.APISERVER
    eps = [W.Endpoint(e.namespace, e.name, [int(ip)], e.owner_refs) for e, ip in zip(base.endpoints, ips)]
    return W.Pods(eps, ips, np.arange(len(ips), dtype=np.int64))


@functools.lru_cache(maxsize=None)
def scattered_pods(n: int = 200, seed: int = 5) -> W.Pods:
    """Pods whose IPs are spread over (nearly) as many /16 prefixes as there are pods."""
    base = W.make_pods(n, seed=seed, secondary_frac=0.0)
    rng = np.random.default_rng(seed)
    ips = np.unique(rng.integers(1, 2**32 - 1, 2 * n, dtype=np.uint64).astype(np.uint32))
    ips = rng.permutation(ips)[:n]
    assert len(np.unique(ips & np.uint32(0xFFFF))) > 65
    eps = [W.Endpoint(e.namespace, e.name, [int(ip)], e.owner_refs) for e, ip in zip(base.endpoints, ips)]
    return W.Pods(eps, ips, np.arange(n, dtype=np.int64))


PodsKey = Union[str, Tuple[int, str], Tuple[int, str, int]]


def pods_of(key: PodsKey) -> W.Pods:
    """"scattered", (npfx, layout) or (npfx, layout, per)."""
    if key == "scattered":
        return scattered_pods()
    return pods_in_prefixes(key[0], key[2] if len(key) > 2 else 40, 0, key[1])


# ---- near-miss records ----------------------------------------------------------------
# of a pod IP p (little-endian u32: the last octet is the high byte)
MUTATIONS = (
    ("last octet ^ 1", lambda p: p ^ np.uint32(1 << 24)),           # same /24, another pod or none
    ("last octet ^ 0x80", lambda p: p ^ np.uint32(0x80 << 24)),
    ("third octet := 200", lambda p: (p & np.uint32(0xFF00FFFF)) | np.uint32(200 << 16)),  # same /16, off the run
    ("third octet ^ 1", lambda p: p ^ np.uint32(1 << 16)),          # the /24 next door, or a hole
    ("second octet ^ 1", lambda p: p ^ np.uint32(1 << 8)),          # the neighbouring /16
    ("first octet ^ 1", lambda p: p ^ np.uint32(1)),
    ("255.255.255.255", lambda p: np.full_like(p, 0xFFFFFFFF)),     # the empty key of both cuckoo forms
    ("0.0.0.0", lambda p: np.zeros_like(p)),
)
MIN_PER_CLASS, MISS_SHARE = 20, (0.25, 0.75)


def mutate(recs: W.Records, pods: W.Pods, seed: int):
    """About 40 % of the source and of the destination IPs, independently, replaced by one
    of the eight MUTATIONS of a randomly chosen pod IP.  Returns the records and, per
    column, how often each class was applied, plus the share of sources that are no pod."""
    rng = np.random.default_rng(seed)
    cols, counts = {}, {}
    for name in ("src_ip", "dst_ip"):
        a = getattr(recs, name)
        n = len(a)
        hit = rng.random(n) < 0.4
        p = pods.ips[rng.integers(0, len(pods.ips), n)].astype(np.uint32)
        cls = rng.integers(0, len(MUTATIONS), n)
        m = np.select([cls == k for k in range(len(MUTATIONS))], [f(p) for _, f in MUTATIONS]).astype(np.uint32)
        cols[name] = np.where(hit, m, a).astype(np.uint32)
        counts[name] = np.bincount(cls[hit], minlength=len(MUTATIONS))
    out = W.Records(cols["src_ip"], cols["dst_ip"], recs.bytes, recs.meta, recs.ports, recs.dns_id, recs.dns)
    return out, dict(counts=counts, miss_share=float((~np.isin(out.src_ip, pods.ips)).mean()))


def check_mutation_stats(st) -> None:
    """No case degenerates: every class at least MIN_PER_CLASS times in each column, and
    between a quarter and three quarters of the sources no pod."""
    for name, c in st["counts"].items():
        assert (c >= MIN_PER_CLASS).all(), (name, c.tolist())
    assert MISS_SHARE[0] <= st["miss_share"] <= MISS_SHARE[1], st["miss_share"]


def near_miss(recs: W.Records, pods: W.Pods, seed: int) -> W.Records:
    out, st = mutate(recs, pods, seed)
    check_mutation_stats(st)
    return out


@functools.lru_cache(maxsize=None)
def inputs(key: PodsKey, n: int = 4000, seed: int = 0):
    """(pods, near-miss records, mutation statistics) of a pod set; shared, never changed."""
    pods = pods_of(key)
    base = W.gen_records(n, pods, seed=100 + seed, drop_frac=0.2, udp_frac=0.1)
    recs, st = mutate(base, pods, 200 + seed)
    check_mutation_stats(st)
    return pods, recs, st


# ---- the case table ---------------------------------------------------------------------
C1_LOCAL_PORT = [dict(o, source_labels=W.C1_LABELS + ["port"]) for o in W.C1_LOCAL]
SPECS = {"fwd-drop": W.LOCAL_FWD_DROP, "c1-local": W.C1_LOCAL, "c1-remote": W.C1_REMOTE,
         "c1-local-port": C1_LOCAL_PORT}


class Case(NamedTuple):
    id: str
    pods: PodsKey
    spec: str      # key of SPECS
    remote: bool
    flags: int
    align: str     # "vec" | "scalar" (every column one element off) | "ports-off" (the ports column only)
    n: int
    kernel: str    # gpuagg_kernel_name after the batch, as launch_aggregate spells it


def _c(cid, pods, spec, flags, align, kernel, n=4000, remote=False):
    return Case(cid, pods, spec, remote, flags, align, n, kernel)


RUN1, RUN4, RUN5, RUN8, RUN9, RUN64, RUN65 = [(k, "run") for k in PREFIX_COUNTS]
HOLES, EDGES, TOO_WIDE = (1, "holes", 120), (2, "edges"), (4, "too-wide")

# (tier-1 with the forward and the drop group both in LDS is the compile-time signature
# kSigFwdLdsDropLds = (0+1 | 8) | (1+1 | 8) << 4 = 169)
CASES = [
    # -- dense_lds_kernel (W.LOCAL_FWD_DROP): the three LDS images, 8-wide and one-IP probes
    _c("t1-dense-1-vec", RUN1, "fwd-drop", 0, "vec", "dense_lds_kernel<2, true, 169u, 2>"),
    _c("t1-dense-4-scalar", RUN4, "fwd-drop", 0, "scalar", "dense_lds_kernel<2, false, 169u, 2>"),
    _c("t1-dense-holes-vec-tail", HOLES, "fwd-drop", 0, "vec", "dense_lds_kernel<2, true, 169u, 2>", n=4001),
    _c("t1-dense-holes-scalar", HOLES, "fwd-drop", 0, "scalar", "dense_lds_kernel<2, false, 169u, 2>"),
    _c("t1-dense-edges-vec", EDGES, "fwd-drop", 0, "vec", "dense_lds_kernel<2, true, 169u, 2>"),
    _c("t1-dense-edges-scalar", EDGES, "fwd-drop", 0, "scalar", "dense_lds_kernel<2, false, 169u, 2>"),
    _c("t1-row-flag-1-vec", RUN1, "fwd-drop", ROW_RADIX, "vec", "dense_lds_kernel<2, true, 169u, 1>"),
    _c("t1-row-flag-4-scalar", RUN4, "fwd-drop", ROW_RADIX, "scalar", "dense_lds_kernel<2, false, 169u, 1>"),
    _c("t1-row-too-wide-vec-tail", TOO_WIDE, "fwd-drop", 0, "vec", "dense_lds_kernel<2, true, 169u, 1>", n=4002),
    _c("t1-row-too-wide-scalar", TOO_WIDE, "fwd-drop", 0, "scalar", "dense_lds_kernel<2, false, 169u, 1>"),
    _c("t1-row-edges-vec", EDGES, "fwd-drop", ROW_RADIX, "vec", "dense_lds_kernel<2, true, 169u, 1>"),
    _c("t1-cuckoo-flag-1-vec", RUN1, "fwd-drop", CUCKOO, "vec", "dense_lds_kernel<2, true, 169u, 0>"),
    _c("t1-cuckoo-flag-4-scalar", RUN4, "fwd-drop", CUCKOO, "scalar", "dense_lds_kernel<2, false, 169u, 0>"),
    _c("t1-cuckoo-5-vec-tail", RUN5, "fwd-drop", 0, "vec", "dense_lds_kernel<2, true, 169u, 0>", n=4003),
    _c("t1-cuckoo-5-scalar", RUN5, "fwd-drop", 0, "scalar", "dense_lds_kernel<2, false, 169u, 0>"),
    _c("t1-cuckoo-scattered-vec", "scattered", "fwd-drop", 0, "vec", "dense_lds_kernel<2, true, 169u, 0>"),
    # only the ports column off a 16-byte boundary: vector loads as long as no group reads it
    _c("t1-ports-off-unread", RUN4, "fwd-drop", 0, "ports-off", "dense_lds_kernel<2, true, 169u, 2>"),
    _c("agg-ports-off-read", RUN4, "c1-local-port", 0, "ports-off", "aggregate_kernel<false, false>"),
    # -- dense_local_kernel (W.LOCAL_FWD_DROP, no LDS image): the three HBM forms
    _c("dl-compare-1-vec", RUN1, "fwd-drop", NO_LDS, "vec", "dense_local_kernel<2, true, false, 0u>"),
    _c("dl-compare-8-vec-tail", RUN8, "fwd-drop", NO_LDS, "vec", "dense_local_kernel<2, true, false, 0u>", n=4003),
    _c("dl-compare-8-scalar", RUN8, "fwd-drop", NO_LDS, "scalar", "dense_local_kernel<2, false, false, 0u>"),
    _c("dl-pre-9-vec", RUN9, "fwd-drop", NO_LDS, "vec", "dense_local_kernel<2, true, false, 0u>"),
    _c("dl-pre-9-scalar", RUN9, "fwd-drop", NO_LDS, "scalar", "dense_local_kernel<2, false, false, 0u>"),
    _c("dl-pre-64-vec", RUN64, "fwd-drop", NO_LDS, "vec", "dense_local_kernel<2, true, false, 0u>"),
    _c("dl-pre-64-scalar", RUN64, "fwd-drop", NO_LDS, "scalar", "dense_local_kernel<2, false, false, 0u>"),
    _c("dl-bucket-65-vec", RUN65, "fwd-drop", NO_LDS, "vec", "dense_local_kernel<2, true, false, 0u>"),
    _c("dl-bucket-65-scalar", RUN65, "fwd-drop", NO_LDS, "scalar", "dense_local_kernel<2, false, false, 0u>"),
    _c("dl-bucket-scattered-vec", "scattered", "fwd-drop", NO_LDS, "vec", "dense_local_kernel<2, true, false, 0u>"),
    _c("dl-bucket-flag-4-scalar", RUN4, "fwd-drop", NO_LDS | NO_RADIX, "scalar",
       "dense_local_kernel<2, false, false, 0u>"),
    # -- aggregate_kernel (W.C1_LOCAL; with vector loads and the wide-key lists the plan
    #    goes to wide_kernel, so the vector rows turn the lists off): the three HBM forms
    _c("agg-compare-4-vec", RUN4, "c1-local", NO_WIDE_LISTS, "vec", "aggregate_kernel<true, false>"),
    _c("agg-compare-8-scalar", RUN8, "c1-local", 0, "scalar", "aggregate_kernel<false, false>"),
    _c("agg-pre-9-vec-tail", RUN9, "c1-local", NO_WIDE_LISTS, "vec", "aggregate_kernel<true, false>", n=4001),
    _c("agg-pre-64-scalar", RUN64, "c1-local", 0, "scalar", "aggregate_kernel<false, false>"),
    _c("agg-bucket-65-vec", RUN65, "c1-local", NO_WIDE_LISTS, "vec", "aggregate_kernel<true, false>"),
    _c("agg-bucket-65-scalar", RUN65, "c1-local", 0, "scalar", "aggregate_kernel<false, false>"),
    _c("agg-bucket-scattered-scalar", "scattered", "c1-local", 0, "scalar", "aggregate_kernel<false, false>"),
    # -- wide_kernel: local context probes the HBM table (4 IPs a lane) ...
    _c("wide-local-pre-9", RUN9, "c1-local", 0, "vec", "wide_kernel<2, false, true, -1>"),
    _c("wide-local-bucket-65", RUN65, "c1-local", 0, "vec", "wide_kernel<2, false, true, -1>"),
    # ... remote context (W.C1_REMOTE) the all-pods LDS image, or the HBM table without one
    _c("wide-dense-4", RUN4, "c1-remote", 0, "vec", "wide_kernel<2, true, true, 2>", remote=True),
    _c("wide-dense-holes-tail", HOLES, "c1-remote", 0, "vec", "wide_kernel<2, true, true, 2>", n=4002, remote=True),
    _c("wide-dense-edges", EDGES, "c1-remote", 0, "vec", "wide_kernel<2, true, true, 2>", remote=True),
    _c("wide-row-flag-1", RUN1, "c1-remote", ROW_RADIX, "vec", "wide_kernel<2, true, true, 1>", remote=True),
    _c("wide-row-too-wide", TOO_WIDE, "c1-remote", 0, "vec", "wide_kernel<2, true, true, 1>", remote=True),
    _c("wide-cuckoo-flag-4", RUN4, "c1-remote", CUCKOO, "vec", "wide_kernel<2, true, true, 0>", remote=True),
    _c("wide-cuckoo-5", RUN5, "c1-remote", 0, "vec", "wide_kernel<2, true, true, 0>", remote=True),
    _c("wide-cuckoo-65-tail", RUN65, "c1-remote", 0, "vec", "wide_kernel<2, true, true, 0>", n=4003, remote=True),
    _c("wide-hbm-compare-1", RUN1, "c1-remote", NO_LDS, "vec", "wide_kernel<2, true, true, -1>", remote=True),
    _c("wide-hbm-pre-9", RUN9, "c1-remote", NO_LDS, "vec", "wide_kernel<2, true, true, -1>", remote=True),
    _c("wide-hbm-bucket-65", RUN65, "c1-remote", NO_LDS, "vec", "wide_kernel<2, true, true, -1>", remote=True),
    # unaligned columns in remote context: no wide_kernel, the generic kernel and the HBM table
    _c("remote-scalar-4", RUN4, "c1-remote", 0, "scalar", "aggregate_kernel<false, false>", remote=True),
    _c("remote-scalar-64", RUN64, "c1-remote", 0, "scalar", "aggregate_kernel<false, false>", remote=True),
]
assert len({c.id for c in CASES}) == len(CASES)


@functools.lru_cache(maxsize=None)
def want_series(key: PodsKey, n: int, spec: str, remote: bool):
    """The oracle's series of a case's inputs: computed once, shared by the backends."""
    pods, recs, _ = inputs(key, n)
    return oracle_series(recs, pods, SPECS[spec], remote)


def offset_columns(ts, which):
    """Device columns moved one element past their 16-byte boundary where `which` says."""
    import torch
    out = []
    for i, t in enumerate(ts):
        if which(i):
            t = torch.cat([t.new_zeros(1), t])[1:]
            assert t.data_ptr() % 16 == 4
        else:
            assert t.data_ptr() % 16 == 0
        out.append(t)
    return out


PORTS_COLUMN = 4  # position in helpers.to_device's list


def device_columns(recs: W.Records, device: int, align: str):
    """(gpuagg columns, the tensors that must outlive the launch)."""
    from retina_amd import GpuAgg
    which = {"vec": lambda i: False, "scalar": lambda i: True, "ports-off": lambda i: i == PORTS_COLUMN}[align]
    ts = offset_columns(to_device(recs, device), which)
    return GpuAgg.device_columns(*ts), ts


def make_case_engine(pods, spec, remote, flags, device=None, recs=None, **kw):
    """device None: the CPU backend."""
    from retina_amd import GpuAgg
    kw.setdefault("max_slots", len(pods.endpoints) + 64)
    kw.setdefault("max_ips", max(16, len(pods.ips)))
    kw.setdefault("sparse_capacity_log2", 16)
    # (the default wide-key lists are 32 GiB of device memory: seconds to allocate, now and then)
    kw.setdefault("wide_list_mib", 64)
    g = GpuAgg(device=device or 0, remote_context=remote, flags=flags | (CPU if device is None else 0), **kw)
    try:
        g.reconcile(spec)
        g.load_endpoints(pods.endpoints)
        if recs is not None:
            intern_dns(g, recs)
    except Exception:
        g.close()
        raise
    return g


def submit(g, recs: W.Records, device, align: str = "vec"):
    """One synced batch: device-resident on a GPU, host-fed on the CPU backend."""
    if device is None:
        g.submit_numpy(recs)
        return
    cols, keep = device_columns(recs, device, align)
    g.submit_device(cols, len(recs))
    g.sync()
    del keep


def run_case(case: Case, device=None):
    """(series, kernel name, stats) of one case on `device` (None: the CPU backend)."""
    pods, recs, _ = inputs(case.pods, case.n)
    g = make_case_engine(pods, SPECS[case.spec], case.remote, case.flags, device, recs)
    try:
        submit(g, recs, device, case.align)
        return g.snapshot(), g.kernel_name(), g.stats()
    finally:
        g.close()


# ---- table swaps across forms -------------------------------------------------------------
# Three generations of the same pods (names and slots stay, every IP moves): in the "run"
# layout an address of generation k belongs to another pod -- or to none -- in generation
# k + 1, so a lookup through anything left of the old table gives a wrong series.
SWAPS = {
    # dense radix image -> cuckoo image -> dense radix image with other prefixes and runs
    "lds": (0, [(4, "run", 50), (5, "run", 40), (1, "run", 200)]),
    # HBM radix by compares -> through the `pre` table -> cuckoo buckets
    "hbm": (NO_LDS, [(8, "run", 585), (9, "run", 520), (65, "run", 72)]),
}
SWAP_N = 3000


@functools.lru_cache(maxsize=None)
def swap_batches(kind: str):
    """[(pods, records)] per generation: near-miss records of the generation's pods, a
    tenth of whose addresses are pod IPs of the generation before."""
    out, prev = [], None
    for gen, key in enumerate(SWAPS[kind][1]):
        pods, recs, _ = inputs(key, SWAP_N, seed=10 + gen)
        if prev is not None:
            rng = np.random.default_rng(300 + gen)
            cols = []
            for a in (recs.src_ip, recs.dst_ip):
                old = prev.ips[rng.integers(0, len(prev.ips), len(a))]
                cols.append(np.where(rng.random(len(a)) < 0.1, old, a).astype(np.uint32))
            recs = W.Records(cols[0], cols[1], recs.bytes, recs.meta, recs.ports, recs.dns_id, recs.dns)
        out.append((pods, recs))
        prev = pods
    assert len({len(p.endpoints) for p, _ in out}) == 1
    return out


@functools.lru_cache(maxsize=None)
def want_swap(kind: str, spec: str, remote: bool):
    """The oracle through the same sequence: the old endpoints deleted, the new ones
    updated into its cache between the batches (cache.go:204-233, 315-337)."""
    from oracle import oracle as O
    from oracle import records as R
    module = O.Module(remote_context=remote)
    module.reconcile(R.spec_from_json(SPECS[spec]))
    cache, prev = O.Cache(), None
    for pods, recs in swap_batches(kind):
        for e in (prev.endpoints if prev is not None else []):
            cache.delete_retina_endpoint(e.namespace + "/" + e.name)
        for e in pods.endpoints:
            cache.update_retina_endpoint(O.RetinaEndpoint(
                name=e.name, namespace=e.namespace, ipv4=O.int2ip(e.ips[0]), other_ipv4s=[],
                owner_refs=None if e.owner_refs is None else [O.Workload(k, n) for k, n in e.owner_refs]))
        R.replay(R.Batch(recs.src_ip, recs.dst_ip, recs.bytes, recs.meta, recs.ports, recs.dns_id), cache, module)
        prev = pods
    return module.series()


def run_swap(kind: str, spec: str, remote: bool, device=None):
    """One engine through the three generations, load_endpoints(version=2) and (version=3)
    between the batches: (series, kernel name after each batch, stats)."""
    flags, _ = SWAPS[kind]
    gens = swap_batches(kind)
    g = make_case_engine(gens[0][0], SPECS[spec], remote, flags, device)
    names = []
    try:
        for gen, (pods, recs) in enumerate(gens):
            if gen:
                for e in gens[gen - 1][0].endpoints:
                    g.cache_delete_endpoint(e.namespace, e.name)
                g.load_endpoints(pods.endpoints, version=gen + 1)
            submit(g, recs, device)
            names.append(g.kernel_name())
        return g.snapshot(), names, g.stats()
    finally:
        g.close()


# ---- the sketch pass's source lookups ---------------------------------------------------------
# launch_sketch: sketch_stage_kernel<kIp, .> with kIp 3 dense radix, 2 row radix, 1 cuckoo
# image of every pod IP, 0 the HBM table (radix always through `pre`, or buckets); columns
# off their 16-byte boundary take sketch_scatter_kernel<false, kLdsIp>, which probes an
# image only in its cuckoo form.
HLL_CASES = [  # (id, pods, flags, unaligned columns, sketch kernel)
    ("dense-4", RUN4, 0, False, "sketch_stage_kernel<3, 0>"),
    ("dense-holes", HOLES, 0, False, "sketch_stage_kernel<3, 0>"),
    ("dense-edges", EDGES, 0, False, "sketch_stage_kernel<3, 0>"),
    ("row-flag-4", RUN4, ROW_RADIX, False, "sketch_stage_kernel<2, 0>"),
    ("row-too-wide", TOO_WIDE, 0, False, "sketch_stage_kernel<2, 0>"),
    ("cuckoo-flag-1", RUN1, CUCKOO, False, "sketch_stage_kernel<1, 0>"),
    ("cuckoo-5", RUN5, 0, False, "sketch_stage_kernel<1, 0>"),
    ("cuckoo-5-unaligned", RUN5, 0, True, "sketch_scatter_kernel<false, true>"),
    ("hbm-pre-9", RUN9, NO_LDS, False, "sketch_stage_kernel<0, 0>"),
    ("hbm-bucket-65-unaligned", RUN65, NO_LDS, True, "sketch_scatter_kernel<false, false>"),
]


@functools.lru_cache(maxsize=None)
def hll_inputs(key: PodsKey, unaligned: bool):
    """A case's near-miss records (4001 of them with unaligned columns: a ragged end), four
    of whose sources are the apiserver pseudo pod: it is a source pod for the HLL."""
    pods, base, _ = inputs(key, 4001 if unaligned else 4000)
    src = base.src_ip.copy()
    src[40:44] = pods.ips[0]
    return pods, W.Records(src, base.dst_ip, base.bytes, base.meta, base.ports, base.dns_id, base.dns)
