"""Segment lists at their capacity and at the device-decided fold's threshold (wide_append,
sparse_fold_wide_kernel's conditional fold, CompactLists, sparse_insert's compact branch and
the fill-counter clamps of sp_counts_out and of the kernels' prologues), written once and run on
both backends: test_seglist_cases_cpu.py (GPUAGG_FLAG_CPU_BACKEND, host-fed: that backend has
no lists, so it validates the inputs, the references and the geometry) and
test_gpu_seglist_cases.py (gfx950, device-resident submits with no sync() between them, every
kernel asserted by name).

Geometry.  blocks, chunk, sp_cap, sp_nwin, budget, accum, fold_cond and the kernel's name are
the real planner's (gpuagg_launch_plan.h through tests/launch_plan_test.cpp), fed with the case's
facts and the device's CU count; nothing here restates list_geom.

Fills.  Every case asserts its per-workgroup list fills from the batch alone, in numpy
(`fills_of`): workgroup b takes records [b * chunk, (b + 1) * chunk), chunk =
((n + blocks - 1) / blocks + 3) & ~3, and a record's key lands in the list of segment
(key_hash & mask) >> seg_log2 (wide) or compact_home >> seg_log2 (compact).  The key words are
the engine's own: one CPU-backend probe run with one record per flow, record i carrying i + 1
bytes (wide; a compact key: i + 1 records, DNS families count no bytes), and sparse_export
identifies the flow by that word.  fmix64 / key_hash are restated in numpy and pinned against
tests/key_hash_test.cpp by the CPU tests.

Why a record is exactly one append, with the hot-key cache on or off.  The wide inputs are
remote-context plans over pod -> pod forwarded records in which every live record makes one
update per forward group (asserted: the reference's counts sum to the live records times the
groups), and inside one workgroup's chunk every key is distinct.  A key enters the LDS cache only
through wide_insert's claim (gpuagg_kernels.hip: `claim = (atomicOr(&s.door[...]) >> ...) & 1u`,
then `if (claim && atomicCAS(&fe->tag, 0ULL, 1ULL) == 0ULL)`): its doorkeeper bit has to be set
already, by an earlier sighting in this workgroup and launch (the bitmap is zeroed in the
kernel's prologue).  With distinct keys that is a false positive of the bitmap only, and such a
key still leaves the cache as exactly one entry (count 1) at the flush loop after the record
loop (`if (e.tag == 2ULL) wide_append(g, ...)`); every other record reaches
`wide_append(s, kh, k0, k1, k2, 1, b)` at the end of wide_insert.  So a workgroup's list of a
segment takes one entry per record of that segment, up to sp_cap; the rest takes
wide_append's `sparse_add` in place.  A chunk is padded to its multiple of 4 with records that
match no group (retransmissions under a forward / drop spec; asserted: their reference is
empty).  Case 5 alone repeats keys on purpose; there the fills are lower bounds.

What the device then does with the fills (`Lists`) -- clamp, threshold, per-segment fold or
keep -- is stated once from sparse_fold_wide_kernel / sp_counts_out and only used to assert that
an input reaches the state its case is named for; results never depend on it."""

from __future__ import annotations

import functools
import subprocess
import zlib
from typing import Dict, List, Optional

import numpy as np

from oracle.ref_cpu import values_only
from retina_amd import _abi
from retina_amd import workloads as W

from . import dense_cases as D
from . import host_programs
from .delta_cases import Acc
from .growth_inputs import ref_series, take, wide_field_rows
from .helpers import diff_series, make_engine, oracle_series, to_device

CPU, PER_BATCH = _abi.FLAG_CPU_BACKEND, _abi.FLAG_FOLD_PER_BATCH
NARROW, NO_HOT, NO_LISTS = _abi.FLAG_NARROW_ENTRIES, _abi.FLAG_NO_HOT_KEYS, _abi.FLAG_NO_WIDE_LISTS
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
COLS = ("src_ip", "dst_ip", "bytes", "meta", "ports", "dns_id")
FWD, DROP, FLAGS, RETRANS, DNS_REQ, DNS_RESP = range(6)
NO_BUDGET = (1 << 63) - 1  # plan_batch: ~0ull >> 1


# ---- hashes (gpuagg_internal.h), in numpy -----------------------------------------------------
def fmix64(k):
    k = np.asarray(k, np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xff51afd7ed558ccd)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xc4ceb9fe1a85ec53)
        k ^= k >> np.uint64(33)
    return k


SEED = np.uint64(0x243F6A8885A308D3)


def key_hash(k0, k1, k2):
    u = np.uint64
    return fmix64(np.asarray(k0, u) ^ fmix64(np.asarray(k1, u) ^ fmix64(np.asarray(k2, u) ^ SEED)))


def compact_hash(key):
    """compact_home before `& mask`."""
    return fmix64(np.asarray(key, np.uint64) ^ SEED)


def host_hashes(keys: np.ndarray):
    """(key_hash, compact hash of k0) of (n, 3) u64 keys by tests/key_hash_test.cpp."""
    exe = host_programs.build("key_hash_test")
    text = "\n".join("%d %d %d" % tuple(int(x) for x in k) for k in keys) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
    got = np.array([int(x) for x in out], np.uint64).reshape(-1, 2)
    assert len(got) == len(keys)
    return got[:, 0], got[:, 1]


# ---- backend ----------------------------------------------------------------------------------
class Backend(D.Backend):
    """dense_cases.Backend; the CPU backend stands in for a device of `cus` CUs (the planner
    decides the same geometry for it, the host mirror has no lists).  dry: no engine and no
    reference at all -- the inputs, their fills and the planner's geometry only."""

    def __init__(self, device=None, cus: int = 256, dry: bool = False):
        super().__init__(device)
        self._cus, self.dry = cus, dry

    @property
    def cus(self) -> int:
        return super().cus if self.gpu else self._cus

    def engine(self, pods, spec, flags=0, recs=None, remote=False, **kw):
        if not self.gpu:
            return make_engine(pods, spec, remote, recs=recs, flags=CPU | flags, **kw)
        return make_engine(pods, spec, remote, self.device, recs, flags=flags, **kw)

    def entries(self, g) -> np.ndarray:
        cap = int(g.state().sparse_len)
        if not self.gpu:
            out = np.zeros((cap, 5), np.uint64)
            return out[:g.sparse_export(out.ctypes.data, cap)]
        import torch
        out = torch.empty((cap, 5), dtype=torch.int64, device=torch.device("cuda", self.device))
        n = g.sparse_export(out.data_ptr(), cap)
        return out[:n].cpu().numpy().view(np.uint64)

    def import_entries(self, g, ent: np.ndarray):
        ent = np.ascontiguousarray(ent)
        if not self.gpu:
            g.sparse_import(ent.ctypes.data, len(ent))
            return
        import torch
        t = torch.from_numpy(ent.view(np.int64)).to(torch.device("cuda", self.device))
        g.sparse_import(t.data_ptr(), len(ent))


def concat(parts) -> W.Records:
    parts = list(parts)
    return W.Records(*[np.concatenate([getattr(p, c) for p in parts]) for c in COLS], parts[0].dns)


_REF: Dict[tuple, dict] = {}


def reference(pods, recs: W.Records, spec, remote: bool) -> dict:
    """{(metric, label values): value}: the oracle per flow, the C port above 50,000 records;
    computed once per input (the variants of a case share theirs)."""
    key = (id(pods), remote, repr(spec), len(recs)) + tuple(zlib.crc32(getattr(recs, c).tobytes()) for c in COLS)
    if key not in _REF:
        if len(recs) <= D.ORACLE_MAX:
            _REF[key] = values_only(oracle_series(recs, pods, spec, remote))
        else:
            _REF[key] = ref_series(pods, recs, spec, remote)
    return _REF[key]


def counted(series: dict) -> int:
    return sum(v for (metric, _), v in series.items() if metric.endswith("_count"))


def total_bytes(series: dict) -> int:
    return sum(v for (metric, _), v in series.items() if metric.endswith("_bytes"))


# ==== wide keys ================================================================================
WIDE_LOG2, WIDE_SEG_LOG2, WIDE_LIST_MIB = 13, 12, 1  # two segments of 2^12 slots; 1 MiB of lists
WIDE_ENGINE = dict(sparse_capacity_log2=WIDE_LOG2, wide_list_mib=WIDE_LIST_MIB)
WIDE_PODS = 64
A, B = 0, 1

_IP = ["ip"]
WIDE_SPECS = {
    "two": W.C1_REMOTE,  # a forward and a drop group: wide_kernel<2, true, true, .>
    # two forward and two drop groups (a metric name has one label set: the counts by address, the
    # bytes by C1's labels): wide_kernel<4, true, false, .>, two updates a record
    "four": W.C1_REMOTE + [{"metric_name": m, "source_labels": _IP, "destination_labels": _IP}
                           for m in ("forward_count", "drop_count")],
    # what `reconcile` changes to: other keys for the same records
    "ip": [{"metric_name": m, "source_labels": _IP, "destination_labels": _IP} for m in ("forward_count", "forward_bytes")],
}
WIDE_FAMILIES = {"two": (FWD, DROP), "four": (FWD, DROP, FWD, DROP), "ip": (FWD,)}
UPDATES = {"two": 1, "four": 2, "ip": 1}  # forward groups: the updates of a live record
POOL_FLOWS = {"two": 1100, "four": 520}  # flows of a kind kept (the table's segments stay below half full)


@functools.lru_cache(maxsize=None)
def wide_pods():
    return W.make_pods(WIDE_PODS, seed=900)


@functools.lru_cache(maxsize=None)
def more_pods():
    """wide_pods() and 16 more."""
    pods, big = wide_pods(), W.make_pods(WIDE_PODS + 16, seed=900)
    new = big.ip_owner >= WIDE_PODS
    return W.Pods(pods.endpoints + big.endpoints[WIDE_PODS:], np.concatenate([pods.ips, big.ips[new]]),
                  np.concatenate([pods.ip_owner, big.ip_owner[new]]))


def _row():
    """(meta, ports) of growth_inputs.wide_field_rows' forwarded pod -> pod record."""
    _, rows = wide_field_rows()
    assert (int(rows.meta[0]) >> 8) & 0xFF == W.V_FWD
    return np.uint32(rows.meta[0]), np.uint32(rows.ports[0])


class Pool:
    """The flows of one spec: every ordered pair of the pods' primary addresses (the apiserver
    pseudo pod left out), their key words from the probe, and per flow `vec` = its updates'
    entries by segment (A, B).  kinds: the flows of each vec, POOL_FLOWS of them at most."""

    def __init__(self, spec_id: str):
        u = np.uint32
        self.spec_id, self.spec, self.pods = spec_id, WIDE_SPECS[spec_id], wide_pods()
        self.groups = UPDATES[spec_id]
        prim = np.array([e.ips[0] for e in self.pods.endpoints[1:]], u)
        s, d = np.meshgrid(prim, prim, indexing="ij")
        ok = s != d
        self.src, self.dst = s[ok].astype(u), d[ok].astype(u)
        n = len(self.src)
        assert n == (WIDE_PODS - 1) * (WIDE_PODS - 2)
        self.meta, self.ports = _row()
        probe = self.records(np.arange(n), np.arange(1, n + 1))
        g = make_engine(self.pods, self.spec, True, flags=CPU, **WIDE_ENGINE)
        try:
            g.submit_numpy(probe)
            ent = Backend().entries(g)
        finally:
            g.close()
        assert len(ent) == n * self.groups and (ent[:, 3] == 1).all(), (len(ent), n)
        flow = ent[:, 4].astype(np.int64) - 1
        order = np.argsort(flow, kind="stable")
        ent, flow = ent[order], flow[order]
        assert (flow == np.repeat(np.arange(n), self.groups)).all()
        self.keys = ent[:, :3].reshape(n, self.groups, 3)  # [flow][update] = (k0, k1, k2)
        assert len({tuple(k) for k in ent[:, :3].tolist()}) == len(ent)
        h = key_hash(ent[:, 0], ent[:, 1], ent[:, 2])
        self.hash = h.reshape(n, self.groups)
        seg = ((h & np.uint64((1 << WIDE_LOG2) - 1)) >> np.uint64(WIDE_SEG_LOG2)).astype(np.int64).reshape(n, self.groups)
        self.vec = np.stack([(seg == A).sum(1), (seg == B).sum(1)], 1)
        self.kinds, self.spare = {}, {}  # spare: four more of each kind, never picked (case 5's hot keys)
        for v in sorted({tuple(x) for x in self.vec.tolist()}):
            fl, k = np.flatnonzero((self.vec == v).all(1)), POOL_FLOWS[spec_id]
            assert len(fl) >= k + 4, (v, len(fl))
            self.kinds[v], self.spare[v] = fl[:k], fl[k:k + 4]
        self.lookup = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(self.src, self.dst))}

    def records(self, flows, nbytes) -> W.Records:
        """One record per entry of `flows`; -1: a padding record (a retransmission: no group)."""
        u = np.uint32
        flows = np.asarray(flows, np.int64)
        live = flows >= 0
        f = np.where(live, flows, 0)
        pad = W.pack_meta(W.PROTO_TCP, W.V_RETRANS, 2, 0, W.ACK)
        return W.Records(self.src[f], self.dst[f], np.asarray(nbytes, u), np.where(live, self.meta, u(pad)).astype(u),
                         np.full(len(f), self.ports, u), np.zeros(len(f), u))

    def pick(self, a: int, b: int, rot: int) -> np.ndarray:
        """Distinct flows whose entries are exactly (a, b), from a rotating start."""
        def some(kind, k):
            fl = self.kinds[kind]
            assert k <= len(fl), (kind, k, len(fl))
            return fl[(rot * 7 + np.arange(k)) % len(fl)]
        if self.groups == 1:
            return np.concatenate([some((1, 0), a), some((0, 1), b)])
        assert (a - b) % 2 == 0, "two entries a record: the fills of a workgroup differ by an even number"
        z = a % 2
        return np.concatenate([some((2, 0), (a - z) // 2), some((0, 2), (b - z) // 2), some((1, 1), z)])

    def flows_of(self, recs: W.Records) -> np.ndarray:
        """The flow of every record, from its addresses and verdict alone; -1: padding."""
        live = ((recs.meta >> np.uint32(8)) & np.uint32(0xFF)) == W.V_FWD
        return np.array([self.lookup[(int(s), int(d))] if ok else -1
                         for s, d, ok in zip(recs.src_ip, recs.dst_ip, live)], np.int64)


@functools.lru_cache(maxsize=None)
def pool(spec_id: str) -> Pool:
    return Pool(spec_id)


def fills_of(p: Pool, recs: W.Records, blocks: int, chunk: int) -> np.ndarray:
    """(blocks, 2): the entries workgroup b appends per segment, from the batch alone; asserts
    that no key repeats inside a chunk."""
    fl = p.flows_of(recs)
    wg = np.arange(len(fl)) // chunk
    assert wg[-1] < blocks
    live = fl >= 0
    pair = wg[live] * len(p.src) + fl[live]
    assert len(np.unique(pair)) == len(pair), "a key repeats inside a workgroup's chunk"
    out = np.zeros((blocks, 2), np.int64)
    np.add.at(out, wg[live], p.vec[fl[live]])
    return out


def build_launch(p: Pool, fills: np.ndarray, seed: int, extra=None) -> W.Records:
    """blocks chunks, chunk b of distinct flows with exactly fills[b] entries (A, B), shuffled,
    padded to the longest chunk's multiple of 4.  extra: per workgroup more flows, repeats
    allowed (case 5's hot keys), mixed in."""
    rng = np.random.default_rng(seed)
    rows = []
    for b, (fa, fb) in enumerate(fills.tolist()):
        fl = p.pick(fa, fb, seed * 131 + b)
        if extra is not None:
            fl = np.concatenate([fl, extra[b]])
        rows.append(rng.permutation(fl))
    chunk = (max(len(r) for r in rows) + 3) & ~3
    chunk = max(chunk, 4)
    flows = np.full((len(rows), chunk), -1, np.int64)
    for b, r in enumerate(rows):
        at = np.sort(rng.choice(chunk, len(r), replace=False))  # padding anywhere in the chunk
        flows[b, at] = r
    flat = flows.reshape(-1)
    nbytes = (np.arange(len(flat)) * 37 + seed) % 1461 + 40
    return p.records(flat, nbytes)


class Lists:
    """The stored fills of every (workgroup, segment) list across launches, as the device
    keeps them: sp_counts_out clamps to sp_cap; a conditional fold (threshold T = sp_cap / 2)
    runs when the fullest list reached T, folds and zeroes the segments with a list at T or
    beyond and keeps the others; an unconditional fold (thr 0) empties every list."""

    def __init__(self, blocks: int, sp_cap: int, cond: bool):
        self.fill = np.zeros((blocks, 2), np.int64)
        self.cap, self.T, self.cond = sp_cap, sp_cap // 2, cond
        self.log: List[dict] = []

    def launch(self, add: np.ndarray) -> dict:
        start = self.fill.copy()
        total = start + add
        ev = dict(start=start, total=total, in_place=np.maximum(total - self.cap, 0) - np.maximum(start - self.cap, 0))
        self.fill = np.minimum(total, self.cap)
        mx = self.fill.max(0)
        ev["folded"] = [bool(m >= self.T) if self.cond else bool(m) for m in mx]
        ev["kept"] = [bool(m) and not f for m, f in zip(mx, ev["folded"])]
        for s in (A, B):
            if ev["folded"][s]:
                self.fill[:, s] = 0
        self.log.append(ev)
        return ev

    def fold_all(self):
        self.fill[:] = 0


# (flags, unaligned columns)
WIDE_VARIANTS = {"default": (0, False), "narrow": (NARROW, False), "no-hot": (NO_HOT, False), "unaligned": (0, True),
                 # the same inputs through the runs that never touch the paths under test
                 "per-batch": (PER_BATCH, False), "no-lists": (NO_LISTS, False)}
# what 2^20 bytes of lists give at 256 CUs: 32-byte (narrow: 24-byte) entries over blocks * 2 lists
SP_CAP_256 = {0: (256, 64), NARROW: (256, 84), NO_HOT: (1024, 16)}


def wide_plan(spec_id: str, cus: int, flags: int, m: int, unaligned: bool = False, pend: Optional[dict] = None) -> dict:
    """The planner's decision for one launch of m records."""
    fams = WIDE_FAMILIES[spec_id]
    words = ["g=%d:1:1:0:1:0" % f for f in fams]
    facts = dict(local=0, remote=1, sparse_slots=1 << WIDE_LOG2, seg_log2=WIDE_SEG_LOG2,
                 wide_list_bytes=WIDE_LIST_MIB << 20, narrow=bool(flags & NARROW), no_hot_keys=bool(flags & NO_HOT),
                 no_wide_lists=bool(flags & NO_LISTS), defer_folds=not flags & PER_BATCH, n_cu=cus, m=m,
                 aligned=0 if unaligned else 63, **{"img_all.bytes": D.ipl_dense_bytes(wide_pods()), "img_all.form": 2})
    for k, v in (pend or {}).items():
        facts["pend." + k] = v
    words += ["%s=%d" % (k, int(v)) for k, v in facts.items()]
    return host_programs.plan(host_programs.planner(), [" ".join(words)])[0]


def wide_name(spec_id: str, flags: int, unaligned: bool) -> str:
    """What the planner has to name for the variant (asserted against it in every run)."""
    if unaligned:
        return "aggregate_kernel<false, false>"
    if flags & (NO_HOT | NO_LISTS):
        return "aggregate_kernel<true, false>"
    n = len(WIDE_FAMILIES[spec_id])
    return "wide_kernel<%d, true, %s, 2>" % (4 if n > 2 else 2, "true" if n == len(set(WIDE_FAMILIES[spec_id])) else "false")


class Geo:
    """blocks, sp_cap and T of a variant on `cus` CUs; the fills are sized with the geometry of
    the variant's list flags (per-batch and no-lists runs take the default variant's inputs)."""

    def __init__(self, spec_id: str, cus: int, flags: int):
        r = wide_plan(spec_id, cus, flags & (NARROW | NO_HOT), 4 * cus)
        self.blocks, self.cap, self.nwin = r["blocks"], r["sp_cap"], r["sp_nwin"]
        self.T = self.cap // 2
        assert self.nwin == 2 and r["fold_cond"] == 1 and r["budget"] == NO_BUDGET and r["defer"] == 1, r
        assert self.cap >= 16 and self.cap % 2 == 0
        if cus == 256:
            assert (self.blocks, self.cap) == SP_CAP_256[flags & (NARROW | NO_HOT)], r


class WideRun:
    """One engine of one variant: launches built from fills, each asserted from its batch and
    against the planner, then submitted unsynced; snapshots against the reference of the
    records so far."""

    def __init__(self, be: Backend, spec_id: str, variant: str, what: str, pods=None, **kw):
        self.be, self.p, self.what, self.variant = be, pool(spec_id), "%s %s %s" % (what, spec_id, variant), variant
        self.flags, self.unaligned = WIDE_VARIANTS[variant]
        self.geo = Geo(spec_id, be.cus, self.flags)
        self.lists_on = not self.flags & (PER_BATCH | NO_LISTS)
        self.lists = Lists(self.geo.blocks, self.geo.cap, cond=True)
        self.spec_id, self.spec, self.pods = spec_id, self.p.spec, pods or self.p.pods
        self.g = None if be.dry else be.engine(self.pods, self.spec, self.flags, remote=True, **dict(WIDE_ENGINE, **kw))
        self.keep, self.sent, self.pend, self.seed = [], [], None, zlib.crc32(what.encode()) & 0xFFFF
        self.want: dict = {}
        self.owed: list = []
        self.names = set()

    def close(self):
        if self.g is not None:
            self.g.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- launches ---------------------------------------------------------------------------
    def fills(self, a, b) -> np.ndarray:
        """(blocks, 2) from two scalars or per-workgroup arrays."""
        out = np.zeros((self.geo.blocks, 2), np.int64)
        out[:, A], out[:, B] = a, b
        return out

    def build(self, fills: np.ndarray, extra=None, exact: bool = True) -> W.Records:
        self.seed += 1
        recs = build_launch(self.p, fills, self.seed, extra)
        blocks = self.geo.blocks
        assert len(recs) % blocks == 0
        chunk = len(recs) // blocks
        if exact:
            got = fills_of(self.p, recs, blocks, chunk)
            assert (got == fills).all(), (got[:4], fills[:4])
        return recs

    def submit(self, recs: W.Records, pods=None, spec_id=None) -> dict:
        """Plans the launch, submits it unsynced, books it in the reference and in `Lists`."""
        blocks = self.geo.blocks
        chunk = len(recs) // blocks
        r = wide_plan(spec_id or self.spec_id, self.be.cus, self.flags, len(recs), self.unaligned, self.pend)
        assert r["chunk"] == chunk and r["blocks"] == blocks and chunk * blocks == len(recs), (r, chunk)
        name = wide_name(spec_id or self.spec_id, self.flags, self.unaligned)
        assert r["name"] == name, (r["name"], name)
        if self.lists_on:
            assert (r["fold_cond"], r["defer"], r["sp_cap"], r["budget"]) == (1, 1, self.geo.cap, NO_BUDGET), r
            assert r["accum"] == (self.pend is not None), (r, self.pend)
            self.pend = dict(active=1, sp_nwin=r["sp_nwin"], sp_cap=r["sp_cap"], budget=r["budget"], blocks=blocks,
                             same_state=1, rpb=(self.pend["rpb"] if self.pend else 0) + chunk)
        else:
            assert r["fold_cond"] == 0 and r["accum"] == 0 and r["sp_nwin"] == (0 if self.flags & NO_LISTS else 2), r
        if self.be.dry:
            return r
        self.keep.append(self.be.submit(self.g, recs, self.unaligned))
        got = self.g.kernel_name()
        self.names.add(got)
        if self.be.gpu:
            assert got == name, (self.what, got, name)
        self.sent.append(recs)
        self.owed.append((pods or self.pods, spec_id or self.spec_id, recs))
        return r

    def settle(self):
        """Books the launches since the last read in the reference: the runs of one cache and
        spec as one batch each."""
        while self.owed:
            pods, spec_id, _ = self.owed[0]
            k = next((i for i, o in enumerate(self.owed) if o[0] is not pods or o[1] != spec_id), len(self.owed))
            recs, self.owed = concat(o[2] for o in self.owed[:k]), self.owed[k:]
            one = reference(pods, recs, WIDE_SPECS[spec_id], True)
            # every live record counts once and with its bytes, the padding not at all (a metric name
            # has one label set, so "four"'s second forward group shows in the byte series; that a
            # record is one entry per forward group is the probe's assertion)
            live = self.p.flows_of(recs) >= 0
            live_bytes = int(recs.bytes[live].astype(np.uint64).sum())
            assert (counted(one), total_bytes(one)) == (int(live.sum()), live_bytes), (counted(one), total_bytes(one))
            self.want = D.add_series(self.want, one)

    def launch(self, a, b, extra=None, exact=True) -> dict:
        """One launch adding (a, b) entries to every workgroup's lists; -> what `Lists` saw."""
        fills = self.fills(a, b)
        self.submit(self.build(fills, extra, exact))
        return self.lists.launch(fills)

    # -- reads ------------------------------------------------------------------------------
    def host_folded(self):
        """A state read: fold_pending folds every list, nothing is pending after it."""
        self.pend = None
        self.lists.fold_all()

    def check(self, what=""):
        if self.be.dry:
            return self.host_folded()
        self.settle()
        got = values_only(self.g.snapshot())
        self.host_folded()
        self.keep.clear()
        dropped = (self.g.last_dropped, self.g.stats()["sparse_dropped"])
        assert dropped == (0, 0) and got == self.want, "%s %s: dropped %s; %s" % (
            self.what, what, dropped, diff_series(got, self.want))
        assert self.want, self.what

    def check_keys(self):
        """The exported key set is the probe's, for the flows submitted."""
        if self.be.dry:
            return
        ent = self.be.entries(self.g)
        self.host_folded()
        fl = np.unique(np.concatenate([self.p.flows_of(r) for r in self.sent]))
        want = {tuple(k) for k in self.p.keys[fl[fl >= 0]].reshape(-1, 3).tolist()}
        got = {tuple(k) for k in ent[:, :3].tolist()}
        assert got == want, (self.what, len(got), len(want))

    def done(self):
        self.check("final")
        self.check_keys()
        print("%s: %s blocks=%d sp_cap=%d" % (self.what, sorted(self.names) if self.be.gpu else "(host) expects " + wide_name(
            self.spec_id, self.flags, self.unaligned), self.geo.blocks, self.geo.cap))


def _even(spec_id: str, a, b):
    """four: two entries a record, so a workgroup's fills differ by an even number -- B one less
    where they would not."""
    if spec_id == "four":
        b = b - ((np.asarray(a) - np.asarray(b)) % 2)
    return a, b


# ---- 1. below ---------------------------------------------------------------------------------
def wide_below(be: Backend, variant: str, spec_id: str = "two"):
    """Three launches to (T - 1, T - 1): no fold fires, the snapshot folds everything."""
    with WideRun(be, spec_id, variant, "below") as r:
        T = r.geo.T
        parts = [(T - 1) // 3, (T - 1) // 3, T - 1 - 2 * ((T - 1) // 3)]
        for k in parts:
            ev = r.launch(k, k)
            assert ev["folded"] == [False, False] and (ev["in_place"] == 0).all()
        assert (r.lists.fill == T - 1).all() and T - 1 > 0
        r.done()


# ---- 2. at the threshold ----------------------------------------------------------------------
THRESHOLD = [("T", "first"), ("T+1", "first"), ("T", "last")]


def wide_threshold(be: Backend, variant: str, at: str, who: str, spec_id: str = "two"):
    """Launch 1: (T, T - 1) -- or T + 1 -- in one workgroup, (T - 1, T - 1) in all others: the
    grid folds, A is folded and zeroed, B kept.  Launch 2 appends 5 to each segment: behind B's
    kept entries, and from 0 in A."""
    with WideRun(be, spec_id, variant, "threshold %s %s" % (at, who)) as r:
        T, blocks = r.geo.T, r.geo.blocks
        a = np.full(blocks, T - 1)
        a[0 if who == "first" else blocks - 1] = T + (at == "T+1")
        a, b = _even(spec_id, a, np.full(blocks, T - 1))
        ev = r.launch(a, b)
        assert ev["folded"] == [True, False] and ev["kept"] == [False, True] and (ev["in_place"] == 0).all()
        assert (r.lists.fill[:, A] == 0).all() and r.lists.fill[:, B].min() >= T - 2 > 0
        a2, b2 = _even(spec_id, 5, 5)
        ev = r.launch(a2, b2)
        assert (ev["start"][:, A] == 0).all() and (ev["start"][:, B] >= T - 2).all()
        # B reaches T + 4 behind its kept entries: the second launch's fold takes B alone
        assert ev["folded"] == [False, True] and ev["total"][:, B].max() < r.geo.cap
        r.done()


# ---- 3. capacity in one launch ------------------------------------------------------------------
def wide_capacity(be: Backend, variant: str, spec_id: str = "two"):
    """A reaches sp_cap - 1, sp_cap, sp_cap + 1 or 3 * sp_cap by workgroup % 4, B one entry:
    everything past sp_cap goes to the table in place."""
    with WideRun(be, spec_id, variant, "capacity") as r:
        cap, w = r.geo.cap, np.arange(r.geo.blocks)
        a = np.choose(w % 4, [cap - 1, cap, cap + 1, 3 * cap])
        a, b = _even(spec_id, a, np.ones(len(w), np.int64))
        ev = r.launch(a, np.maximum(b, 0))
        assert sorted(set(ev["in_place"][:, A].tolist())) == [0, 1, 2 * cap]
        assert (r.lists.fill[:, A] == 0).all() and ev["folded"][A]
        r.done()


# ---- 4. capacity behind a kept list -------------------------------------------------------------
def wide_capacity_behind(be: Backend, variant: str, spec_id: str = "two"):
    """(T - 1, T - 1) as in `below`, then one launch adds sp_cap to B only: the append crosses
    sp_cap mid-launch, from a stored fill that is not zero."""
    with WideRun(be, spec_id, variant, "capacity-behind") as r:
        T, cap = r.geo.T, r.geo.cap
        for k in ((T - 1) // 2, T - 1 - (T - 1) // 2):
            r.launch(k, k)
        assert (r.lists.fill == T - 1).all()
        ev = r.launch(0, cap)
        assert (ev["start"][:, B] == T - 1).all() and (ev["in_place"][:, B] == T - 1).all() and T - 1 > 0
        assert ev["folded"] == [False, True] and ev["kept"] == [True, False]
        r.done()


# ---- 5. counted entries at a full list ----------------------------------------------------------
HOT_REPEATS = 300


def wide_counted(be: Backend, variant: str, spec_id: str = "two"):
    """Cold distinct keys fill A to sp_cap; three hot keys (two of A, one of B), each 300 times a
    chunk, are flushed from the cache as entries of count > 1: B's goes into B's list, A's find A
    full.  (A hot key's first sightings are 1-count appends, so the fills are lower bounds
    here: A is full either way.)  With FLAG_NO_HOT_KEYS every update is a 1-count entry."""
    with WideRun(be, spec_id, variant, "counted") as r:
        cap, p = r.geo.cap, r.p
        hot = np.concatenate([p.spare[(1, 0)][:2], p.spare[(0, 1)][:1]])
        fills = r.fills(cap, 3)
        recs = r.build(fills, extra=[np.repeat(hot, HOT_REPEATS)] * r.geo.blocks, exact=False)
        fl = p.flows_of(recs).reshape(r.geo.blocks, -1)
        cold = np.where(np.isin(fl, hot), -1, fl)
        for row in cold:  # the cold keys alone: distinct, exactly sp_cap of A in every chunk
            live = row[row >= 0]
            assert len(set(live.tolist())) == len(live) and (p.vec[live].sum(0) == [cap, 3]).all()
        assert ((fl[:, :, None] == hot).sum(1) == HOT_REPEATS).all() and HOT_REPEATS < 4096  # (the entry's count field)
        r.submit(recs)
        r.done()


# ---- 6. many folds ------------------------------------------------------------------------------
MANY_LAUNCHES, MANY_SNAPSHOTS = 40, (13, 26)


def wide_many_folds(be: Backend, variant: str, spec_id: str = "two"):
    """40 launches alternate which segment takes T / 2 + 1 entries: a segment folds on every
    second launch it takes, on alternating flag words; two snapshots in between (the
    unconditional fold_pending_dense) and the final one each against the records so far."""
    with WideRun(be, spec_id, variant, "many-folds") as r:
        k = r.geo.T // 2 + 1
        k += k % 2 if spec_id == "four" else 0
        folds = []
        for i in range(MANY_LAUNCHES):
            ev = r.launch(k if i % 2 == A else 0, k if i % 2 == B else 0)
            assert (ev["in_place"] == 0).all()
            if any(ev["folded"]):
                folds.append((i, ev["folded"].index(True), i % 2))
            if i + 1 in MANY_SNAPSHOTS:
                r.check("after launch %d" % (i + 1))
        assert len(folds) >= 12 and {f[1] for f in folds} == {A, B} and {f[2] for f in folds} == {0, 1}, folds
        assert any(sum(ev["kept"]) for ev in r.lists.log)
        r.done()


# ---- 7. operations while a list is kept ---------------------------------------------------------
def _kept(r: WideRun):
    """Case 2's state after launch 1: A folded on the device, B kept at T - 1, pend active."""
    T, blocks = r.geo.T, r.geo.blocks
    a = np.full(blocks, T - 1)
    a[0] = T
    ev = r.launch(*_even(r.spec_id, a, np.full(blocks, T - 1)))
    assert ev["folded"] == [True, False] and ev["kept"] == [False, True]
    assert r.pend is not None or not r.lists_on


def op_reset(be: Backend, variant: str):
    with WideRun(be, "two", variant, "op reset") as r:
        _kept(r)
        r.g.reset()
        r.host_folded()
        r.want, r.sent, r.owed = {}, [], []
        r.launch(5, 5)
        r.done()


def op_reconcile(be: Backend, variant: str):
    """To another wide spec: the table is cleared, the kept list dropped; the same records are
    other keys under the new spec."""
    with WideRun(be, "two", variant, "op reconcile") as r:
        _kept(r)
        r.g.reconcile(WIDE_SPECS["ip"])
        r.host_folded()
        r.want, r.sent, r.owed = {}, [], []
        recs = r.build(r.fills(5, 5))
        r.submit(recs, spec_id="ip")
        r.settle()
        got = values_only(r.g.snapshot())
        assert r.g.last_dropped == 0 and r.g.stats()["sparse_dropped"] == 0
        assert got == r.want and got, diff_series(got, r.want)


def op_delta(be: Backend, variant: str):
    """snapshot_delta before and after launch 2: the accumulated deltas equal the snapshot."""
    with WideRun(be, "two", variant, "op delta") as r:
        acc = Acc(r.g)
        _kept(r)
        _, reb = acc.step()
        r.host_folded()
        assert reb
        acc.check()
        r.launch(5, 5)
        _, reb = acc.step()
        r.host_folded()
        assert not reb
        acc.check()
        r.settle()
        assert values_only(acc.acc) == r.want, diff_series(values_only(acc.acc), r.want)
        r.done()


def op_export_import(be: Backend, variant: str):
    """sparse_export with a list kept, sparse_import into a second engine: both hold launch 1;
    the first goes on with launch 2."""
    with WideRun(be, "two", variant, "op export") as r, WideRun(be, "two", variant, "op import") as s:
        _kept(r)
        ent = be.entries(r.g)
        r.host_folded()
        be.import_entries(s.g, ent)
        r.settle()
        s.want, s.sent = dict(r.want), list(r.sent)
        s.done()
        r.launch(5, 5)
        r.done()


def op_merge(be: Backend, variant: str):
    """merge_from of a second engine in the same kept state: the single engine over both inputs."""
    with WideRun(be, "two", variant, "op merge") as r, WideRun(be, "two", variant, "op merge, other") as s:
        _kept(r)
        _kept(s)
        r.g.merge_from([s.g])
        r.host_folded()
        s.host_folded()
        r.settle()
        s.settle()
        r.want, r.sent = D.add_series(r.want, s.want), r.sent + s.sent
        assert s.g.snapshot() == {}  # gpuagg_merge resets the engines it folded in
        r.launch(5, 5)
        r.done()


def op_more_pods(be: Backend, variant: str):
    """load_endpoints with 16 more pods under the kept list; launch 2 under the larger cache."""
    more = more_pods()
    with WideRun(be, "two", variant, "op more-pods", max_slots=len(more.endpoints) + 64, max_ips=len(more.ips) + 64) as r:
        _kept(r)
        r.g.load_endpoints(more.endpoints[WIDE_PODS:])
        recs = r.build(r.fills(5, 5))
        r.submit(recs, pods=more)
        r.lists.launch(r.fills(5, 5))
        r.done()


def op_retire(be: Backend, variant: str):
    """A third of the pods is deleted and retire_slots() rebuilds the table under the kept list;
    launch 2 without the gone pods' rows (delta_cases.retire).  What the gone pods counted
    leaves the snapshot with them."""
    with WideRun(be, "two", variant, "op retire") as r:
        _kept(r)
        gone = [e for i, e in enumerate(r.pods.endpoints) if i % 3 == 1]
        gone_ips = np.array([ip for e in gone for ip in e.ips], np.uint32)
        gone_names = {e.name for e in gone}
        for e in gone:
            r.g.cache_delete_endpoint(e.namespace, e.name)
        r.g.cache_commit(2)
        assert r.g.retire_slots() == len(gone)
        r.host_folded()
        recs = r.build(r.fills(5, 5))
        stays = ~(np.isin(recs.src_ip, gone_ips) | np.isin(recs.dst_ip, gone_ips))
        live = r.p.flows_of(recs) >= 0
        assert 0 < (stays & live).sum() < live.sum()
        recs = take(recs, np.flatnonzero(stays))
        r.keep.append(be.submit(r.g, recs, r.unaligned))
        r.settle()
        r.want = D.add_series(r.want, reference(r.pods, recs, r.spec, True))
        r.want = {k: v for k, v in r.want.items() if not gone_names & set(k[1])}
        got = values_only(r.g.snapshot())
        assert r.g.last_dropped == 0 and r.g.stats()["sparse_dropped"] == 0
        assert got == r.want and got, diff_series(got, r.want)


def op_growth(be: Backend, variant: str):
    """set_sparse_growth turned on (up to 2^16 slots) under the kept list, then a launch of 4,400
    new keys: the table of 2^13 slots is more than half full and doubles, so sp_nwin changes
    under the pending geometry.  ("four": two keys a flow.)"""
    with WideRun(be, "four", variant, "op growth") as r:
        _kept(r)
        r.g._check(r.g.lib.gpuagg_set_sparse_growth(r.g.h, 16, 0))
        p, blocks = r.p, r.geo.blocks
        fl = np.arange(2200)  # each once, dealt over the workgroups
        assert 2 * len(fl) > 1 << (WIDE_LOG2 - 1) and 2 * (len(fl) + sum(len(k) for k in p.kinds.values())) < 1 << WIDE_LOG2
        chunk = (-(-len(fl) // blocks) + 3) & ~3
        flows = np.full(blocks * chunk, -1, np.int64)
        flows[:len(fl)] = fl
        recs = p.records(flows, np.arange(len(flows)) % 1461 + 40)
        r.keep.append(be.submit(r.g, recs, r.unaligned))
        r.want = D.add_series(r.want, reference(r.pods, recs, r.spec, True))
        r.sent.append(recs)
        r.check("grown")
        info = r.g.sparse_info()
        print("op growth %s: %s" % (variant, info))
        assert info["capacity_log2"] == WIDE_LOG2 + 1 and info["grows"] == 1, info
        r.launch(*_even("four", 5, 5))  # the lists of the grown table: four segments
        r.check("after")


WIDE_OPS = {"reset": op_reset, "reconcile": op_reconcile, "delta": op_delta, "export-import": op_export_import,
            "merge": op_merge, "more-pods": op_more_pods, "retire": op_retire, "growth": op_growth}


# ==== compact keys =============================================================================
# The default table of 2^20 slots: 128 segments of 2^13.  A DNS query from a pod to an address
# that is no pod's is one update of the plan's request group (local context: the source side),
# one compact key per (pod, query); no cache stands before these lists, so every such record is
# one append whether its key repeats or not.
COMPACT_LOG2, COMPACT_SEG_LOG2 = D.SPARSE_CAPACITY_LOG2, D.SPARSE_SEG_LOG2
COMPACT_SEGS = (1 << COMPACT_LOG2) >> COMPACT_SEG_LOG2
COMPACT_PLANS = ["dns-only", "dns-two", "c5-small", "c5-staged"]
COMPACT_PODS, COMPACT_QUERIES = 150, 4
EXT = W.ip_le(100, 64, 0, 1)


class CompactPool:
    """The keys of one plan of dense_cases.PLANS: pods 1 .. 150 x 4 queries, key and segment of
    each from the probe (key i submitted i + 1 times: its count names it), and TCP records
    between pods for the plans with dense groups."""

    def __init__(self, plan: str):
        u = np.uint32
        spec_id, n_pods, _, _ = D.PLANS[plan]
        self.plan, self.spec, self.pods = plan, D.SPECS[spec_id], D.pods_of(n_pods)
        self.dns = [W.DnsPayload(0, ["A"], "q%d.example.com" % q, [], 0) for q in range(COMPACT_QUERIES)]
        pod = np.repeat(np.arange(1, COMPACT_PODS + 1), COMPACT_QUERIES)
        self.src = np.array([self.pods.endpoints[i].ips[0] for i in pod], u)
        self.q = np.tile(np.arange(COMPACT_QUERIES), COMPACT_PODS).astype(u)
        assert EXT not in set(self.pods.ips.tolist())
        n = len(pod)
        _, tcp = D.mixed(n_pods, 4096, False, 7)
        self.tcp = tcp
        probe = self.records(np.repeat(np.arange(n), np.arange(1, n + 1)))
        g = make_engine(self.pods, self.spec, False, recs=probe, flags=CPU)
        try:
            g.submit_numpy(probe)
            ent = Backend().entries(g)
        finally:
            g.close()
        assert len(ent) == n and (ent[:, 1] == 0).all(), (len(ent), n)
        ent = ent[np.argsort(ent[:, 3])]
        assert (ent[:, 3] == np.arange(1, n + 1)).all()
        self.key = ent[:, 0] | (ent[:, 2] & np.uint64(0xFFFFFFFF))  # sparse_add: k0 | (k2 & 0xFFFFFFFF)
        assert len(set(self.key.tolist())) == n
        self.hash = compact_hash(self.key)
        self.seg = ((self.hash & np.uint64((1 << COMPACT_LOG2) - 1)) >> np.uint64(COMPACT_SEG_LOG2)).astype(np.int64)
        self.lookup = {(int(s), int(q)): i for i, (s, q) in enumerate(zip(self.src, self.q))}

    def records(self, items) -> W.Records:
        """items >= 0: a query of that key; -1 - j: row j of the TCP records."""
        u = np.uint32
        items = np.asarray(items, np.int64)
        dns = items >= 0
        k, t = np.where(dns, items, 0), np.where(dns, 0, -1 - items) % len(self.tcp)
        meta = W.pack_meta(W.PROTO_UDP, W.V_DNS, 2, dns_type=1)
        return W.Records(np.where(dns, self.src[k], self.tcp.src_ip[t]).astype(u),
                         np.where(dns, u(EXT), self.tcp.dst_ip[t]).astype(u),
                         np.where(dns, u(100), self.tcp.bytes[t]).astype(u),
                         np.where(dns, u(meta), self.tcp.meta[t]).astype(u),
                         np.where(dns, u(40000 | (53 << 16)), self.tcp.ports[t]).astype(u),
                         np.where(dns, self.q[k], u(0)).astype(u), self.dns)

    def fills_of(self, recs: W.Records, blocks: int, chunk: int) -> np.ndarray:
        """(blocks, 128): the keys workgroup b appends per segment, from the batch alone."""
        is_dns = ((recs.meta >> np.uint32(8)) & np.uint32(0xFF)) == W.V_DNS
        out = np.zeros((blocks, COMPACT_SEGS), np.int64)
        at = np.flatnonzero(is_dns)
        keys = np.array([self.lookup[(int(recs.src_ip[i]), int(recs.dns_id[i]))] for i in at], np.int64)
        np.add.at(out, (at // chunk, self.seg[keys]), 1)
        return out

    def of_segment(self, seg: int) -> np.ndarray:
        return np.flatnonzero(self.seg == seg)

    def busiest(self, k: int = 2):
        """The k segments with the most keys of the universe."""
        return np.argsort(-np.bincount(self.seg, minlength=COMPACT_SEGS), kind="stable")[:k].tolist()


@functools.lru_cache(maxsize=None)
def compact_pool(plan: str) -> CompactPool:
    return CompactPool(plan)


def compact_plan(plan: str, cus: int, flags: int, m: int, unaligned: bool, pend: Optional[dict]) -> dict:
    geo = D.plan_geometry(plan, 0)
    words = ["g=%d:%d:%d:%d:%d:%d" % (g.fam, g.sparse, g.nsub, g.base, g.keyed, g.nbins) for g in geo.groups]
    facts = dict(dense_len=geo.dense_len, need_dns=1, compact=1, sparse_slots=1 << COMPACT_LOG2, n_cu=cus, m=m,
                 aligned=0 if unaligned else 63, defer_folds=not flags & PER_BATCH)
    for k, v in (pend or {}).items():
        facts["pend." + k] = v
    words += ["%s=%d" % (k, int(v)) for k, v in facts.items()]
    return host_programs.plan(host_programs.planner(), [" ".join(words)])[0]


class CompactRun:
    """One engine of one plan: every launch planned by the real planner (chunk, sp_cap, budget,
    accum, the name against dense_cases.kernel_name), its fills asserted from the batch, then
    submitted unsynced.  `fill`: the entries every (workgroup, segment) list was asked to take
    since the last host fold; `in_place`: those past sp_cap."""

    def __init__(self, be: Backend, plan: str, unaligned: bool, what: str, flags: int = 0):
        self.be, self.p, self.unaligned, self.flags = be, compact_pool(plan), unaligned, flags
        self.what = "%s %s%s f%d" % (what, plan, " unaligned" if unaligned else "", flags)
        geo = D.plan_geometry(plan, flags)
        self.name = D.kernel_name(geo, vec=not unaligned)
        if not unaligned:
            assert self.name == D.PLANS[plan][2]
        self.blocks = be.cus if geo.dense_len else 4 * be.cus
        self.g = None if be.dry else be.engine(self.p.pods, self.p.spec, flags, recs=self.p.records([0]))
        self.pend, self.keep, self.sent, self.folds = None, [], [], 0
        self.fill = np.zeros((self.blocks, COMPACT_SEGS), np.int64)
        self.cap = 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        if self.g is not None:
            self.g.close()

    def plan_for(self, chunk: int) -> dict:
        """What the planner will decide for a launch of `chunk` records a workgroup."""
        return compact_plan(self.p.plan, self.be.cus, self.flags, chunk * self.blocks, self.unaligned, self.pend)

    def submit(self, items: np.ndarray) -> np.ndarray:
        """items: (blocks, chunk).  -> this launch's fills (blocks, 128)."""
        blocks, chunk = items.shape
        assert blocks == self.blocks and chunk % 4 == 0
        recs = self.p.records(items.reshape(-1))
        r = self.plan_for(chunk)
        assert (r["chunk"], r["blocks"], r["sp_nwin"], r["fold_cond"]) == (chunk, blocks, COMPACT_SEGS, 0), r
        assert r["name"] == self.name, (r["name"], self.name)
        assert r["defer"] == (not self.flags & PER_BATCH), r
        if not r["accum"]:  # the host folds what waited (or nothing did)
            self.folds += self.pend is not None
            self.fill[:] = 0
        self.cap = r["sp_cap"]
        got = self.p.fills_of(recs, blocks, chunk)
        self.fill += got
        self.pend = None
        if r["defer"]:
            self.pend = dict(active=1, nwin=r["nwin"], spill_cap=r["spill_cap"], win_blocks=r["win_blocks"],
                             win_shift=r["win_shift"], sp_nwin=r["sp_nwin"], sp_cap=r["sp_cap"], budget=r["budget"],
                             rpb=(r["accum"] and self.rpb or 0) + chunk, blocks=blocks, lds_bins=r["lds_bins"],
                             dense_len=D.plan_geometry(self.p.plan, 0).dense_len, same_state=1,
                             staged=r["stage_defer"], stage_stride=r["stage_stride"])
        self.rpb = self.pend["rpb"] if self.pend else 0
        self.last = r
        if not self.be.dry:
            self.keep.append(self.be.submit(self.g, recs, self.unaligned))
            got_name = self.g.kernel_name()
            if self.be.gpu:
                assert got_name == self.name, (self.what, got_name, self.name)
            self.sent.append(recs)
        if self.flags & PER_BATCH:
            self.fill[:] = 0
        return got

    def done(self):
        if self.be.dry:
            return
        recs = concat(self.sent)
        want = reference(self.p.pods, recs, self.p.spec, False)
        got = values_only(self.g.snapshot())
        assert self.g.last_dropped == 0 and self.g.stats()["sparse_dropped"] == 0, self.what
        assert got == want and want, "%s: %s" % (self.what, diff_series(got, want))
        n_dns = int(((recs.meta >> np.uint32(8)) & np.uint32(0xFF) == W.V_DNS).sum())
        assert sum(v for (m, _), v in want.items() if "dns_request" in m) == n_dns  # one update a query
        print("%s: %s blocks=%d sp_cap=%d budget=%d host folds=%d" % (
            self.what, self.g.kernel_name() if self.be.gpu else "(host) expects " + self.name, self.blocks, self.cap,
            self.last["budget"], self.folds))

    def spread(self, rng, n: int, avoid=()) -> np.ndarray:
        """n keys of the universe drawn evenly, none of the segments `avoid`."""
        ok = np.flatnonzero(~np.isin(self.p.seg, list(avoid)))
        return ok[rng.integers(0, len(ok), n)]


def compact_overflow(be: Backend, plan: str, unaligned: bool):
    """One DNS key in every record of one launch, 256 records a workgroup: the planner sizes the
    lists for 64 such launches spread evenly (budget 16,384: 128 + 25 % + 64 = 224 at 128
    lists), so every workgroup's last 32 keys find the list full."""
    with CompactRun(be, plan, unaligned, "overflow") as r:
        key = int(r.p.of_segment(r.p.busiest(1)[0])[0])
        got = r.submit(np.full((r.blocks, 256), key, np.int64))
        seg = int(r.p.seg[key])
        assert (got[:, seg] == 256).all() and got.sum() == 256 * r.blocks
        assert (r.last["budget"], r.cap) == (16_384, 224), r.last  # 64 * 256; 128 + 32 + 64
        assert 256 - r.cap == 32
        r.done()


def _capacity_items(r: CompactRun, chunk: int, cap: int, seed: int, mult: int = 2):
    """(blocks, chunk): a hot key of one segment cap - 1, cap, cap + 1 or mult * cap times by
    workgroup % 4, the rest keys of other segments drawn evenly (plans with dense groups: half of
    the rest TCP records)."""
    rng = np.random.default_rng(seed)
    seg = r.p.busiest(1)[0]
    hot = r.p.of_segment(seg)
    items = np.empty((r.blocks, chunk), np.int64)
    counts = []
    for w in range(r.blocks):
        k = (cap - 1, cap, cap + 1, mult * cap)[w % 4]
        assert k <= chunk
        rest = r.spread(rng, chunk - k, avoid=[seg])
        if D.plan_geometry(r.p.plan, 0).dense_len:
            rest = np.where(rng.random(len(rest)) < 0.5, -1 - rng.integers(0, len(r.p.tcp), len(rest)), rest)
        items[w] = rng.permutation(np.concatenate([hot[rng.integers(0, len(hot), k)], rest]))
        counts.append(k)
    return items, seg, np.array(counts)


def compact_capacity(be: Backend, plan: str, unaligned: bool, per_batch: bool = False):
    """One segment's list filled to sp_cap - 1, sp_cap, sp_cap + 1 or 2 * sp_cap by workgroup % 4
    in one launch, the other records keys of other segments.  Deferred, a launch's own budget
    (64 launches of its chunk) gives lists longer than half its chunk, so a launch of 64 records a
    workgroup comes first and fixes the budget (4,096: sp_cap 32 + 8 + 64 = 104), and the launch
    of 256 a workgroup accumulates behind it.  With FLAG_FOLD_PER_BATCH the one launch of 256 is
    alone (budget 256: sp_cap 2 + 64 = 66)."""
    with CompactRun(be, plan, unaligned, "capacity", PER_BATCH if per_batch else 0) as r:
        rng = np.random.default_rng(41)
        seg = r.p.busiest(1)[0]
        if not per_batch:
            first = r.spread(rng, r.blocks * 64, avoid=[seg]).reshape(r.blocks, 64)
            got = r.submit(first)
            assert (got[:, seg] == 0).all() and got.max() < r.cap == 104 and r.last["budget"] == 4096, r.last
            cap = r.plan_for(256)["sp_cap"]
            assert cap == r.cap and r.plan_for(256)["accum"] == 1
        else:
            cap = r.plan_for(256)["sp_cap"]
            assert cap == 66
        items, seg2, counts = _capacity_items(r, 256, cap, 42)
        got = r.submit(items)
        assert seg2 == seg and (got[:, seg] == counts).all() and r.cap == cap
        assert sorted(set((counts - cap).tolist())) == [-1, 0, 1, cap]
        other = np.delete(r.fill if not per_batch else got, seg, axis=1)
        assert other.max() < cap, other.max()  # every other list stays below its capacity
        r.done()


def compact_crossing(be: Backend, plan: str, unaligned: bool):
    """chunk = 64: two launches of one segment's keys cross sp_cap (104) in the second launch,
    from a stored fill of 64; six more start at a full list (the clamp when the fill is read);
    then the snapshot."""
    with CompactRun(be, plan, unaligned, "crossing") as r:
        rng = np.random.default_rng(43)
        seg = r.p.busiest(1)[0]
        hot = r.p.of_segment(seg)
        for i in range(8):
            got = r.submit(hot[rng.integers(0, len(hot), (r.blocks, 64))])
            assert (got[:, seg] == 64).all() and (i == 0 or r.last["accum"] == 1), r.last
            if i == 0:
                assert r.cap == 104 and r.last["budget"] == 4096
            if i == 1:
                assert (r.fill[:, seg] - 64 < r.cap).all() and (r.fill[:, seg] > r.cap).all()
        assert r.folds == 0 and (r.fill[:, seg] == 512).all()
        r.done()


def compact_budget_end(be: Backend, plan: str, unaligned: bool, launches: int):
    """chunk = 4: the budget is 256 records a workgroup (sp_cap 2 + 64 = 66), so the 65th launch
    no longer accumulates (rpb + chunk > budget) and the host folds once -- a list of 256 entries
    asked, full.  70 launches leave 24 entries behind that fold; 134 put a second host fold behind
    another full list, so a full list has a fold on either side."""
    with CompactRun(be, plan, unaligned, "budget-end %d" % launches) as r:
        rng = np.random.default_rng(44)
        seg = r.p.busiest(1)[0]
        hot = r.p.of_segment(seg)
        for i in range(launches):
            before = r.fill[:, seg].copy()
            r.submit(hot[rng.integers(0, len(hot), (r.blocks, 4))])
            assert r.last["accum"] == (i % 64 != 0), (i, r.last)
            if i and i % 64 == 0:
                assert (before == 256).all() and r.cap == 66 and r.last["budget"] == 256
        assert r.folds == (launches - 1) // 64 and (r.fill[:, seg] == 4 * ((launches - 1) % 64 + 1)).all()
        r.done()


def compact_two_hot(be: Backend, unaligned: bool):
    """c5-staged: a launch of 64 records a workgroup fixes the budget (sp_cap 104), then one of
    1,024: one segment's list full (110 keys), another half full (52), the rest sparse -- beside
    TCP records whose tcpflags / retransmit updates go through the spill rings in the same launch."""
    with CompactRun(be, "c5-staged", unaligned, "two-hot") as r:
        rng = np.random.default_rng(45)
        s1, s2 = r.p.busiest(2)
        first = np.where(rng.random((r.blocks, 64)) < 0.5, -1 - rng.integers(0, 4096, (r.blocks, 64)),
                         r.spread(rng, r.blocks * 64, avoid=[s1, s2]).reshape(r.blocks, 64))
        r.submit(first)
        cap = r.cap
        assert cap == 104 and r.plan_for(1024)["accum"] == 1
        h1, h2 = r.p.of_segment(s1), r.p.of_segment(s2)
        items = np.empty((r.blocks, 1024), np.int64)
        for w in range(r.blocks):
            rest = r.spread(rng, 1024 - cap - 6 - cap // 2, avoid=[s1, s2])
            rest = np.where(rng.random(len(rest)) < 0.6, -1 - rng.integers(0, 4096, len(rest)), rest)
            items[w] = rng.permutation(np.concatenate([h1[rng.integers(0, len(h1), cap + 6)],
                                                       h2[rng.integers(0, len(h2), cap // 2)], rest]))
        got = r.submit(items)
        assert (got[:, s1] == cap + 6).all() and (got[:, s2] == cap // 2).all()
        other = np.delete(r.fill, [s1, s2], axis=1)
        assert other.max() < cap // 2 and r.last["staged"] == 1 and r.last["accum"] == 1, (other.max(), r.last)
        r.done()


# ==== the runs =================================================================================
WIDE_CASES = {"below": wide_below, "capacity": wide_capacity, "capacity-behind": wide_capacity_behind,
              "counted": wide_counted, "many-folds": wide_many_folds}
WIDE_CASES.update({"threshold-%s-%s" % (at, who): functools.partial(
    lambda be, variant, spec_id="two", at=at, who=who: wide_threshold(be, variant, at, who, spec_id))
    for at, who in THRESHOLD})
# cases 2, 3 and 6 with the four-group spec
FOUR_CASES = [c for c in WIDE_CASES if c.startswith("threshold") or c in ("capacity", "many-folds")]
GEOMETRY_VARIANTS = ["default", "narrow", "no-hot"]  # the variants with list shapes of their own
WIDE_RUNS = ([(c, v, "two") for c in WIDE_CASES for v in WIDE_VARIANTS] +
             [(c, v, "four") for c in FOUR_CASES for v in GEOMETRY_VARIANTS + ["unaligned"]])
OP_RUNS = [(o, v) for o in WIDE_OPS for v in GEOMETRY_VARIANTS + ["unaligned"]]
COMPACT_CASES = {"overflow": compact_overflow, "capacity": compact_capacity,
                 "capacity-per-batch": lambda be, plan, un: compact_capacity(be, plan, un, True),
                 "crossing": compact_crossing,
                 "budget-end-70": lambda be, plan, un: compact_budget_end(be, plan, un, 70),
                 "budget-end-134": lambda be, plan, un: compact_budget_end(be, plan, un, 134)}
COMPACT_RUNS = [(c, p, u) for c in COMPACT_CASES for p in COMPACT_PLANS for u in (False, True)]


def run_id(run) -> str:
    return "-".join("unaligned" if x is True else "aligned" if x is False else str(x) for x in run)
