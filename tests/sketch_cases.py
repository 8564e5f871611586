"""The sketch-shape cases (launch_sketches / launch_sketch), written once and run on both
backends: test_sketch_shapes_cpu.py (GPUAGG_FLAG_CPU_BACKEND, host-fed: the case tables and
the numpy restatement against the host mirror, Engine::sketch) and test_gpu_sketch_shapes.py
(gfx950, device-resident submits, every scatter kernel asserted by name).

What every case asserts: the count-min rows and the HLL registers of the pods bit-exact
against oracle/sketch.py, every count-min row summing to the number of records, and -- on
the GPU -- gpuagg_sketch_kernel_name, which names the scatter kernel of the last launch
(the folds are launched apart from it and are not part of the name: that a geometry takes
the fold kernels follows from the scatter kernel and the flags, see "Sketch pass" in
DESIGN.md).  Each case prints the name it saw."""

from __future__ import annotations

import functools
import math

import numpy as np

from oracle import sketch as S
from retina_amd import _abi
from retina_amd import workloads as W

from .growth_inputs import take
from .helpers import make_engine, to_device

CPU, PER_BATCH, DIRECT = _abi.FLAG_CPU_BACKEND, _abi.FLAG_FOLD_PER_BATCH, _abi.FLAG_DIRECT_SKETCH
CUCKOO, ROW_RADIX = _abi.FLAG_LDS_CUCKOO, _abi.FLAG_ROW_RADIX
SPEC = [{"metric_name": "forward_count", "source_labels": ["namespace", "podname"]}]


def src_slots(pods, src):
    """The slot (endpoint index) of each source IP, -1 where no pod owns it."""
    ip_slot = {}
    for s, ep in enumerate(pods.endpoints):
        for ip in ep.ips:
            ip_slot[int(ip)] = s
    lut_ips = np.array(sorted(ip_slot), np.uint32)
    lut_slot = np.array([ip_slot[int(x)] for x in lut_ips], np.int64)
    pos = np.clip(np.searchsorted(lut_ips, src), 0, len(lut_ips) - 1)
    return np.where(lut_ips[pos] == src, lut_slot[pos], -1)


# ---- kernel names (launch_sketch) -------------------------------------------------------
def stage(flags: int, d: int, p: int) -> str:
    """sketch_stage_kernel<kIp, kD>: kIp the source lookup (0 HBM table -- no HLL, no
    lookups --, 1 cuckoo, 2 radix, 3 dense radix LDS image), kD 4 or the run-time loop."""
    ip = 0 if not p else 1 if flags & CUCKOO else 2 if flags & ROW_RADIX else 3
    return "sketch_stage_kernel<%d, %d>" % (ip, 4 if d == 4 else 0)


def scatter(vec: bool, flags: int, p: int = 10) -> str:
    """sketch_scatter_kernel<kVec, kLdsIp>: the unstaged kernel probes an LDS image only in
    its cuckoo form."""
    return "sketch_scatter_kernel<%s, %s>" % ("true" if vec else "false",
                                              "true" if p and flags & CUCKOO else "false")


class Backend:
    """device None: the CPU backend, host-fed; else that GPU, device-resident submits."""

    def __init__(self, device=None):
        self.device = device
        self.gpu = device is not None

    @property
    def cus(self) -> int:
        """Scatter workgroups of a launch (one per CU); the host mirror has none: 256."""
        if not self.gpu:
            return 256
        import torch
        return int(torch.cuda.get_device_properties(self.device).multi_processor_count)

    def engine(self, pods, d, w, p, flags=0, **kw):
        kw.setdefault("max_slots", len(pods.endpoints) + 64)
        if not self.gpu:
            return make_engine(pods, SPEC, False, flags=CPU | flags, cms_depth=d, cms_width_log2=w,
                               hll_precision=p, **kw)
        return make_engine(pods, SPEC, False, self.device, flags=flags, cms_depth=d, cms_width_log2=w,
                           hll_precision=p, **kw)

    def submit(self, g, recs, unaligned=False):
        """One unsynced submit.  unaligned: every column starts one element past a 16-byte
        boundary.  Returns what has to stay alive until the engine has read it."""
        if not self.gpu:
            if unaligned:
                cols = [np.concatenate([np.zeros(1, a.dtype), a])[1:]
                        for a in (recs.src_ip, recs.dst_ip, recs.bytes, recs.meta, recs.ports, recs.dns_id)]
                recs = W.Records(*cols)
            g.submit_numpy(recs)
            return None
        from retina_amd import GpuAgg
        ts = to_device(recs, self.device)
        if unaligned:
            import torch
            ts = [torch.cat([t.new_zeros(1), t])[1:] for t in ts]
            assert all(t.data_ptr() % 16 == 4 for t in ts)
        else:
            assert all(t.data_ptr() % 16 == 0 for t in ts)
        g.submit_device(GpuAgg.device_columns(*ts), len(recs))
        return ts


def expected(pods, parts, d, w, p):
    """The numpy restatement over every submitted part: (count-min rows, HLL registers)."""
    want_c = np.zeros((d, 1 << w), np.uint32) if d else None
    want_h = np.zeros((len(pods.endpoints), 1 << p), np.uint8) if p else None
    for r in parts:
        if d:
            S.cms_update(want_c, r.src_ip, r.dst_ip, r.ports, r.meta & np.uint32(0xFF))
        if p:
            S.hll_update(want_h, src_slots(pods, r.src_ip), r.dst_ip, p)
    return want_c, want_h


def verify(g, pods, parts, d, w, p, want=None):
    """The three assertions of every case; returns the restated (rows, registers)."""
    want_c, want_h = want if want is not None else expected(pods, parts, d, w, p)
    n = sum(len(r) for r in parts)
    cms, hll = g.cms_array(), g.hll_array()
    if d:
        assert cms.shape == want_c.shape
        bad = np.flatnonzero((cms != want_c).any(axis=1))
        assert bad.size == 0, "count-min rows %s differ (d=%d w=2^%d, n=%d)" % (bad.tolist(), d, w, n)
        for r in range(d):
            assert int(cms[r].sum()) == n, (r, int(cms[r].sum()), n)
    else:
        assert cms.size == 0
    if p:
        np_ = len(pods.endpoints)
        assert hll.shape[0] >= np_ and hll.shape[1] == 1 << p
        bad = np.flatnonzero((hll[:np_] != want_h).any(axis=1))
        assert bad.size == 0, "HLL registers of %d pods differ (first %s, p=%d)" % (bad.size, bad[:8].tolist(), p)
        assert want_h.any()
    else:
        assert hll.size == 0
    return want_c, want_h


def run(be: Backend, pods, parts, d, w, p, flags=0, name=None, unaligned=False, **kw):
    """One engine, one unsynced submit per part, one read; the scatter kernel's name on the
    GPU (read before the state is compared, asserted after it: a wrong state is the finding,
    the route explains it)."""
    g = be.engine(pods, d, w, p, flags, **kw)
    try:
        keep = [be.submit(g, r, unaligned) for r in parts]
        got = g.sketch_kernel_name()
        print("d=%d w=2^%d p=%d flags=%d n=%d: %s" % (d, w, p, flags, sum(len(r) for r in parts), got or "(host)"))
        verify(g, pods, parts, d, w, p)
        del keep
        if be.gpu and name is not None:
            assert got == name, (got, name)
        return got
    finally:
        g.close()


@functools.lru_cache(maxsize=None)
def inputs(n_pods: int, n: int, seed: int = 0):
    """Seeded pods and records: 80 % of the sources are pods, a fifth of the flows UDP."""
    pods = W.make_pods(n_pods, seed=600 + seed)
    return pods, W.gen_records(n, pods, seed=700 + seed, udp_frac=0.2)


# ---- depth sweep ------------------------------------------------------------------------
# sketch_stage_kernel<kIp, 0> unrolls its run-time depth loop over kStageMaxDepth = 8 rows;
# depths 9..16 take the unstaged kernel, whose loop has no bound of its own (8 and 9: both
# sides of that threshold).
STAGE_MAX_DEPTH = 8
DEPTHS = [(dd, 0) for dd in (1, 2, 3, 5, 8, 9, 16)] + [(3, ROW_RADIX), (3, CUCKOO)]


def depth_sweep(be: Backend, d: int, flags: int):
    pods, recs = inputs(100, 60_000)
    name = stage(flags, d, 10) if d <= STAGE_MAX_DEPTH else scatter(True, flags)
    run(be, pods, [recs], d, 12, 10, flags, name)


# ---- one sketch alone ---------------------------------------------------------------------
def cms_only(be: Backend, d: int):
    """No HLL: no source lookups, kIp = 0; nothing of HLL in the name or the state."""
    pods, recs = inputs(100, 100_000, 1)
    got = run(be, pods, [recs], d, 16, 0, 0, stage(0, d, 0))
    assert "hll" not in got


# p = 4: hll_shift 8, 300 pods in two fine windows of 256; p = 17: hll_shift 0, one pod per
# fine window, 128 slots in 16 super-windows of 8
HLL_ONLY = [(4, 300), (10, 300), (17, 72)]


def hll_only(be: Backend, p: int, n_pods: int):
    """No count-min (depth 0, nwin == 0): the staged kernel with only the HLL rings."""
    pods, recs = inputs(n_pods, 100_000, 2)
    got = run(be, pods, [recs], 0, 0, p, 0, stage(0, 0, p))
    assert "cms" not in got


# ---- narrow rows ----------------------------------------------------------------------
NARROW = [4, 10, 15, 16]  # win_shift = w below 2^15 (one window per row), 15 from there on


def narrow_rows(be: Backend, w: int):
    """w = 2^4: every record of a workgroup lands in the same 16 columns of each row, the
    rings overflow into the lists every round."""
    pods, recs = inputs(100, 100_000, 3)
    run(be, pods, [recs], 4, w, 10, 0, stage(0, 4, 10))


# ---- the staging rings do not fit ---------------------------------------------------------
# stage_words (gpuagg_sketch_plan.h), w = 2^22, one HLL super-window: d = 4 gives 512 windows
# with 128-entry rings, 4 * (1028 + 32772 + 8192 + 64) = 168,224 bytes at round 4 (> 160 KiB)
# but 4 * (1028 + 32772 + 4096 + 64) = 151,840 bytes at round 2, which fits beside an IP
# image of up to 12,000 bytes: that shape is the round-2 fallback, not the unstaged kernel.
# d = 5: 640 windows, the u16 rings alone are 640 * 128 * 2 = 163,840 bytes at either round,
# so no staged launch is possible whatever the image's size.
def rings_do_not_fit(be: Backend, flags: int):
    pods, recs = inputs(100, 100_000, 4)
    run(be, pods, [recs], 5, 22, 10, flags, scatter(True, flags))


def rings_round2(be: Backend):
    """d = 4, w = 2^22 (see above): staged at round 2 when the IP image is small enough,
    else unstaged; gpuagg_sketch_kernel_name does not tell the round, so the name is only
    required to be one of the two."""
    pods, recs = inputs(100, 100_000, 4)
    got = run(be, pods, [recs], 4, 22, 10, 0)
    if be.gpu:
        assert got in (stage(0, 4, 10), scatter(True, 0)), got


# ---- direct paths -------------------------------------------------------------------------
def direct_hll(be: Backend):
    """p = 18 > kHllWindowLog2Bytes: no HLL lists, every register update a global CAS from
    the unstaged kernel; count-min stays windowed (its lists are folded at the read)."""
    pods, recs = inputs(64, 100_000, 5)
    got = run(be, pods, [recs], 4, 12, 18, 0, scatter(True, 0))
    assert "hll_split" not in got and "hll_fold" not in got


def direct_flag(be: Backend):
    """GPUAGG_FLAG_DIRECT_SKETCH: no lists at all (nwin == 0, hnsup == 0), nothing to fold."""
    pods, recs = inputs(100, 100_000, 6)
    got = run(be, pods, [recs], 3, 12, 10, DIRECT, scatter(True, DIRECT))
    assert "fold" not in got


# ---- unaligned columns --------------------------------------------------------------------
UNALIGNED = [(4, 0), (4, CUCKOO), (5, 0), (5, CUCKOO)]


def unaligned(be: Backend, d: int, flags: int):
    """Columns one element past a 16-byte boundary: the scalar-load scatter kernel."""
    pods, recs = inputs(100, 100_003, 7)
    run(be, pods, [recs], d, 12, 10, flags, scatter(False, flags), unaligned=True)


# ---- one set of deferred lists under both kernels -------------------------------------------
def mixed_accumulate(be: Backend):
    """Six unsynced submits, aligned and unaligned in turn, ragged sizes, one read: the
    staged and the scalar-load kernel append to the same deferred lists, each continuing
    from the fill counters the other stored.  With FLAG_FOLD_PER_BATCH every launch folds
    its own lists: both equal the restatement and each other."""
    pods, recs = inputs(100, 200_000, 8)
    sizes = [30_001, 20_003, 40_000, 9_999, 33_333, 12_345]
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    parts = [take(recs, slice(int(a), int(b))) for a, b in zip(bounds[:-1], bounds[1:])]
    want = expected(pods, parts, 4, 12, 10)
    states = []
    for flags in (0, PER_BATCH):
        g = be.engine(pods, 4, 12, 10, flags)
        try:
            keep, names = [], []
            for k, part in enumerate(parts):
                keep.append(be.submit(g, part, unaligned=bool(k & 1)))
                names.append(g.sketch_kernel_name())
            print("flags=%d: %s" % (flags, names))
            verify(g, pods, parts, 4, 12, 10, want)
            states.append((g.cms_array(), g.hll_array()))
            del keep
            if be.gpu:
                assert names == [stage(0, 4, 10), scatter(False, 0)] * 3, names
        finally:
            g.close()
    assert np.array_equal(states[0][0], states[1][0]) and np.array_equal(states[0][1], states[1][1])


# ---- ragged record counts -------------------------------------------------------------------
RAGGED = ["1", "3", "7", "4cu-1", "4cu+1", "1024cu+5"]


def ragged_n(be: Backend, which: str, unaligned_cols: bool):
    """chunk = ((n + B - 1) / B + 3) & ~3 records per workgroup: below 4 * B records the last
    workgroups' chunks start at or past n; n % 4 != 0 splits the last chunk into the vector
    body and the scalar tail (the staged kernel's one-record round)."""
    cu = be.cus
    n = {"1": 1, "3": 3, "7": 7, "4cu-1": 4 * cu - 1, "4cu+1": 4 * cu + 1, "1024cu+5": 1024 * cu + 5}[which]
    pods, recs = inputs(100, 1024 * 256 + 5, 9)
    if n > len(recs):  # more CUs than 256
        pods, recs = inputs(100, n, 9)
    part = take(recs, slice(0, n))
    if n < 8:  # sources that are pods, so the HLL path sees them
        part.src_ip = pods.ips[:n].copy()
    name = scatter(False, 0) if unaligned_cols else stage(0, 4, 10)
    run(be, pods, [part], 4, 12, 10, 0, name, unaligned=unaligned_cols)


# ---- lists that really overflow -------------------------------------------------------------
OVERFLOW_D, OVERFLOW_W, OVERFLOW_P, OVERFLOW_PODS = 1, 18, 14, 200
# 5 * 2^20 records: a count-min list holds mean * 9/8 + 2048 entries, so at a chunk of c
# records per workgroup, 8 windows and half the records on one 5-tuple the busiest list
# takes 9/16 c against a capacity of 9/64 c + 2048 -- twice the capacity needs c >= 14,564,
# i.e. 3.7M records on 256 workgroups (at 1M records, c = 4096, no list can reach twice
# its capacity of 2624 at all).
OVERFLOW_N = 5 << 20


def list_geometry(n: int, blocks: int, d: int, w: int, p: int, hll_slots: int):
    """The list sizing of the sketch planner (gpuagg_sketch_plan.h) under FLAG_FOLD_PER_BATCH,
    restated: sketch_geom and the capacities for one launch's chunk, with
      chunk   = ((n + B - 1) / B + 3) & ~3                       records per workgroup
      nwin    = d << (w - win_shift), win_shift = min(15, w)    count-min windows
      cap     = (mean + mean / 8 + 2048 + 7) & ~7,  mean = chunk * d / nwin
      hshift  = min(8, 17 - p); hsshift grows from hshift while more than 16 super-windows
                remain (and hsshift < 26 - p, < hshift + 10); hnsup = ceil(slots / 2^hsshift)
      hcap    = (mean + mean / 4 + 64 + 15) & ~15,  mean = chunk / hnsup"""
    chunk = ((n + blocks - 1) // blocks + 3) & ~3
    win_shift = min(15, w)
    nwin = d << (w - win_shift)
    mean = chunk * d // nwin
    cap = (mean + mean // 8 + 2048 + 7) & ~7
    hshift = min(8, 17 - p)
    ss = hshift
    while ((hll_slots + (1 << ss) - 1) >> ss) > 16 and ss < 26 - p and ss < hshift + 10:
        ss += 1
    hnsup = (hll_slots + (1 << ss) - 1) >> ss
    hmean = chunk // hnsup
    hcap = (hmean + hmean // 4 + 64 + 15) & ~15
    return dict(chunk=chunk, win_shift=win_shift, nwin=nwin, cap=cap, hsshift=ss, hnsup=hnsup, hcap=hcap)


@functools.lru_cache(maxsize=None)
def overflow_inputs():
    """Half the records one 5-tuple (one count-min column per row), another quarter from the
    same source pod towards distinct destinations (three quarters of the HLL entries in one
    super-window's list, real register updates among them), the rest uniform; the kinds are
    mixed at random, so every workgroup's slice has the same skew."""
    pods = W.make_pods(OVERFLOW_PODS, seed=81)
    n, u = OVERFLOW_N, np.uint32
    rng = np.random.default_rng(82)
    src = pods.ips[rng.integers(0, len(pods.ips), n)].astype(u)
    dst = rng.integers(1, 1 << 32, n, dtype=np.uint64).astype(u)
    ports = (rng.integers(32768, 61000, n, dtype=u) | (u(443) << u(16))).astype(u)
    kind = rng.integers(0, 4, n)
    hot_ip = u(pods.endpoints[37].ips[0])
    src[kind < 3] = hot_ip
    dst[kind < 2] = dst[0]
    ports[kind < 2] = ports[0]
    meta = np.full(n, W.pack_meta(W.PROTO_TCP, W.V_FWD, 1), u)
    recs = W.Records(src, dst, np.full(n, 64, u), meta, ports, np.zeros(n, u))
    want = expected(pods, [recs], OVERFLOW_D, OVERFLOW_W, OVERFLOW_P)
    return pods, recs, want, src_slots(pods, src)


def busiest_lists(recs, slot, geo, blocks: int, d: int, w: int):
    """Entries of the fullest count-min and HLL list over all workgroups' slices."""
    n = len(recs)
    wg = np.arange(n, dtype=np.int64) // geo["chunk"]
    assert int(wg[-1]) < blocks
    lo = recs.src_ip.astype(S.U64) | (recs.dst_ip.astype(S.U64) << S.U64(32))
    hi = recs.ports.astype(S.U64) | ((recs.meta & np.uint32(0xFF)).astype(S.U64) << S.U64(32))
    base = S.fmix64(lo ^ S.fmix64(hi ^ S.CMS_SEED))
    hi_bits = w - geo["win_shift"]
    busiest = 0
    for r in range(d):
        win = (r << hi_bits) | (S.cms_cols(base, r, 1 << w) >> geo["win_shift"])
        busiest = max(busiest, int(np.bincount(wg * geo["nwin"] + win, minlength=blocks * geo["nwin"]).max()))
    ok = slot >= 0
    hbusiest = int(np.bincount(wg[ok] * geo["hnsup"] + (slot[ok] >> geo["hsshift"]),
                               minlength=blocks * geo["hnsup"]).max())
    return busiest, hbusiest


def list_overflow(be: Backend, unaligned_cols: bool):
    """FLAG_FOLD_PER_BATCH: lists sized for this one launch.  Before the engine sees a record
    the sizing rules are restated and the busiest lists counted: one count-min and one HLL
    list take at least twice their capacity, so the past-capacity branches (staged kernel:
    flush and rb + pos; scatter kernel: pos >= cap) carry a large share of the updates."""
    d, w, p = OVERFLOW_D, OVERFLOW_W, OVERFLOW_P
    pods, recs, want, slot = overflow_inputs()
    g = be.engine(pods, d, w, p, PER_BATCH)
    try:
        blocks = be.cus
        geo = list_geometry(len(recs), blocks, d, w, p, int(g.state().hll_len) >> p)
        busiest, hbusiest = busiest_lists(recs, slot, geo, blocks, d, w)
        margin = "count-min list: %d entries / capacity %d (x%.2f); HLL list: %d / %d (x%.2f); %s" % (
            busiest, geo["cap"], busiest / geo["cap"], hbusiest, geo["hcap"], hbusiest / geo["hcap"], geo)
        print(margin)
        assert busiest >= 2 * geo["cap"] and hbusiest >= 2 * geo["hcap"], margin
        keep = be.submit(g, recs, unaligned_cols)
        got = g.sketch_kernel_name()
        print(got or "(host)")
        verify(g, pods, [recs], d, w, p, want)
        del keep
        if be.gpu:
            name = scatter(False, 0) if unaligned_cols else stage(0, d, p)
            assert got == name, (got, name)
    finally:
        g.close()


# ---- estimates --------------------------------------------------------------------------
def cms_estimates(be: Backend, d: int):
    """gpuagg_cms_estimate == the restatement's point query, for 1,000 keys that occur and
    100 that do not (protocol 200 is in no record)."""
    pods, recs = inputs(100, 100_000, 10)
    g = be.engine(pods, d, 12, 0)
    try:
        keep = be.submit(g, recs)
        want_c, _ = verify(g, pods, [recs], d, 12, 0)
        del keep
        g.sketch_refresh()
        proto = recs.meta & np.uint32(0xFF)
        key = np.unique(np.stack([recs.src_ip, recs.dst_ip, recs.ports, proto], 1), axis=0)
        key = key[np.random.default_rng(11).choice(len(key), 1000, replace=False)]
        absent = key[:100].copy()
        absent[:, 3] = 200
        key = np.concatenate([key, absent])
        want = S.cms_estimate(want_c, key[:, 0], key[:, 1], key[:, 2], key[:, 3])
        got = np.array([g.cms_estimate(int(a), int(b), int(c), int(e)) for a, b, c, e in key], np.int64)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
        assert (want[:1000] >= 1).all()
    finally:
        g.close()


HLL_EST_TOL = 1e-9  # both sides sum <= 2^18 doubles in (0, 1]: order differences <= 2^18 * 2^-53 ~ 3e-11


def hll_estimates(be: Backend, p: int):
    """gpuagg_hll_estimate == the restatement's, every pod.  At p = 4 pod 7 has seen three
    destinations (linear counting: m * ln(m / zeros)) and pod 9 thousands (no empty
    register, the raw estimate)."""
    pods, base = inputs(64, 100_000, 12)
    recs = W.Records(base.src_ip.copy(), base.dst_ip.copy(), base.bytes, base.meta, base.ports, base.dns_id)
    few, many = 7, 9
    few_ips = np.array(pods.endpoints[few].ips, np.uint32)
    recs.src_ip[np.isin(recs.src_ip, few_ips)] = pods.endpoints[many].ips[0]
    recs.src_ip[:3] = few_ips[0]
    recs.dst_ip[:3] = np.array([W.ip_le(100, 70, 0, 1), W.ip_le(100, 70, 0, 2), W.ip_le(100, 70, 0, 3)], np.uint32)
    recs.src_ip[1000:6000] = pods.endpoints[many].ips[0]
    recs.dst_ip[1000:6000] = np.random.default_rng(13).integers(1, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32)
    g = be.engine(pods, 4, 12, p)
    try:
        keep = be.submit(g, recs)
        _, want_h = verify(g, pods, [recs], 4, 12, p)
        del keep
        g.sketch_refresh()
        slot = src_slots(pods, recs.src_ip)
        assert len(np.unique(recs.dst_ip[slot == few])) == 3 and len(np.unique(recs.dst_ip[slot == many])) > 2000
        for s in range(len(pods.endpoints)):
            want = S.hll_estimate(want_h[s])
            got = g.hll_estimate(s)
            assert abs(got - want) <= HLL_EST_TOL * want, (s, got, want)
        if p == 4:
            zeros = int((want_h[few] == 0).sum())
            assert 13 <= zeros <= 15
            assert S.hll_estimate(want_h[few]) == 16 * math.log(16 / zeros)
            assert not (want_h[many] == 0).any() and S.hll_estimate(want_h[many]) > 2.5 * 16
    finally:
        g.close()
