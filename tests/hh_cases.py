"""The sketch-readout cases -- heavy-hitter candidates and top-k (gpuagg_set_heavy_hitters,
gpuagg_heavy_hitters, gpuagg_hh_*) and the distinct peers of every pod in one call
(gpuagg_hll_estimate_all) -- written once and run on both backends: test_hh_cpu.py (the CPU
backend, host-fed) and test_gpu_hh.py (gfx950, device-resident submits: hh_candidate_kernel,
hh_rank_kernel, hll_estimate_kernel of gpuagg_hh.hip).

The numpy restatement of the candidate rule, on oracle/sketch.py: per submit, in order,
cms_update; the unique keys of that submit; cms_estimate on them; keys with estimate >= T join
a Python set.  At the end the top-k of the set by (-estimate, key).

Every heavy-hitter case asserts four things (check): set(hh_candidates()) equals the restated
set exactly, with no key twice; heavy_hitters(k) equals the restated top-k exactly for k = 1,
16 and beyond the number of candidates; hh_info's candidates and dropped match; the count-min
rows are still bit-exact (sketch_cases.verify).

The workload (planted): sketch_cases.inputs(100, 60_000, 20) with 48 planted flows of
40 + 25 j records on the rows of default_rng(21).permutation, d = 4.  The width 2^12 is the
clean case; at 2^8 collisions admit false positives, the set depends on how the records are
split into submits (the per-submit rule), and estimates tie around rank 16 (the tie order).
The case functions print the candidate counts they see."""

from __future__ import annotations

import functools
import math

import numpy as np
import pytest

from oracle import sketch as S
from retina_amd import _abi
from retina_amd import workloads as W
from retina_amd.engine import GpuAggError

from . import sketch_cases as K
from .growth_inputs import take

PER_BATCH = _abi.FLAG_FOLD_PER_BATCH
N_PLANTED = 48


def keys_of(r: W.Records) -> np.ndarray:
    """uint32 [n, 4]: the key the count-min hashes (src_ip, dst_ip, ports, proto)."""
    return np.stack([r.src_ip, r.dst_ip, r.ports, r.meta & np.uint32(0xFF)], 1).astype(np.uint32)


def estimate(cms: np.ndarray, keys: np.ndarray) -> np.ndarray:
    keys = np.asarray(keys, np.uint32).reshape(-1, 4)
    if not len(keys):
        return np.zeros(0, np.int64)
    return S.cms_estimate(cms, keys[:, 0], keys[:, 1], keys[:, 2], keys[:, 3])


def restate(parts, d: int, w: int, T: int, test_from: int = 0):
    """(count-min rows, candidate set) after the submits `parts`; only submits test_from..
    are tested (the feature was set after the earlier ones)."""
    cms = np.zeros((d, 1 << w), np.uint32)
    cand = set()
    for i, r in enumerate(parts):
        key = keys_of(r)
        S.cms_update(cms, key[:, 0], key[:, 1], key[:, 2], key[:, 3])
        if i < test_from:
            continue
        uniq = np.unique(key, axis=0)
        for k in uniq[estimate(cms, uniq) >= T]:
            cand.add(tuple(int(x) for x in k))
    return cms, cand


def topk(cms: np.ndarray, cand, k: int):
    """[(src, dst, ports, proto, estimate)] of the k largest by (-estimate, key)."""
    keys = sorted(cand)
    est = estimate(cms, np.array(keys, np.uint32))
    order = sorted(range(len(keys)), key=lambda i: (-int(est[i]), keys[i]))[:k]
    return [keys[i] + (int(est[i]),) for i in order]


def rows(hh: np.ndarray):
    return [(int(e["src_ip"]), int(e["dst_ip"]), int(e["ports"]), int(e["proto"]), int(e["estimate"])) for e in hh]


def candidates(g):
    got = g.hh_candidates()
    as_set = set(tuple(int(x) for x in k) for k in got)
    assert len(as_set) == len(got), "a key twice among %d candidates" % len(got)
    return as_set


def check(g, pods, parts, d, w, p, cms, cand, dropped=0):
    """The four assertions of every case (module docstring)."""
    got = candidates(g)
    assert got == cand, "candidates: %d missing, %d unexpected (of %d restated)" % (
        len(cand - got), len(got - cand), len(cand))
    for k in (1, 16, len(cand) + 5):
        assert rows(g.heavy_hitters(k)) == topk(cms, cand, k), "top-%d" % k
    info = g.hh_info()
    assert info["candidates"] == len(cand) and info["dropped"] == dropped, info
    want = K.expected(pods, parts, d, w, p)
    assert np.array_equal(want[0], cms)
    K.verify(g, pods, parts, d, w, p, want)


@functools.lru_cache(maxsize=None)
def planted():
    pods, base = K.inputs(100, 60_000, 20)
    recs = W.Records(base.src_ip.copy(), base.dst_ip.copy(), base.bytes, base.meta.copy(), base.ports.copy(),
                     base.dns_id)
    perm = np.random.default_rng(21).permutation(len(recs))
    pos = 0
    for j in range(N_PLANTED):
        at = perm[pos:pos + 40 + 25 * j]
        pos += len(at)
        for col in (recs.src_ip, recs.dst_ip, recs.meta, recs.ports):
            col[at] = col[at[0]]
    return pods, recs


def thirds(recs):
    return [take(recs, slice(i, None, 3)) for i in range(3)]


def run(be, pods, parts, d, w, p, T, lg, flags=0, unaligned=False, dropped=0):
    """One engine with the feature on from the start, one unsynced submit per part, the four
    assertions; returns (rows, candidate set, heavy_hitters(16))."""
    cms, cand = restate(parts, d, w, T)
    print("d=%d w=2^%d p=%d T=%d submits=%d flags=%d: %d candidates" % (d, w, p, T, len(parts), flags, len(cand)))
    g = be.engine(pods, d, w, p, flags)
    try:
        g.set_heavy_hitters(T, lg)
        assert g.hh_info() == {"candidates": 0, "dropped": 0, "min_count": T, "capacity_log2": lg or 16}
        keep = [be.submit(g, r, unaligned) for r in parts]
        check(g, pods, parts, d, w, p, cms, cand, dropped)
        del keep
        return cms, cand, rows(g.heavy_hitters(16))
    finally:
        g.close()


# ---- one submit, three submits ------------------------------------------------------------
WIDTHS, THRESHOLDS = (12, 8), (300, 600)
# candidates of the restatement per (width, T, submits): the clean width gives the same set for
# one submit or three, 2^8 columns do not
RESTATED = {(12, 300, 1): 37, (12, 600, 1): 25, (12, 300, 3): 37, (12, 600, 3): 25,
            (8, 300, 1): 105, (8, 600, 1): 63, (8, 300, 3): 88, (8, 600, 3): 45}


def one_submit(be, w: int, T: int):
    pods, recs = planted()
    _, cand, _ = run(be, pods, [recs], 4, w, 10, T, 0)
    assert len(cand) == RESTATED[w, T, 1]
    # every planted flow with at least T records is a candidate (estimates never under-count)
    key, cnt = np.unique(keys_of(recs), axis=0, return_counts=True)
    heavy = set(tuple(int(x) for x in k) for k in key[cnt >= T])
    assert heavy and heavy <= cand
    if w == 8:
        assert len(cand) > len(heavy), "2^8 columns admit no false positive"


def three_submits(be, w: int, T: int):
    """Three interleaved thirds, then the same under FLAG_FOLD_PER_BATCH: deferral must not
    show.  At 2^8 columns the per-submit rule admits fewer keys than one submit does."""
    pods, recs = planted()
    parts = thirds(recs)
    a = run(be, pods, parts, 4, w, 10, T, 0)
    b = run(be, pods, parts, 4, w, 10, T, 0, PER_BATCH)
    assert a[1] == b[1] and a[2] == b[2]
    assert len(a[1]) == RESTATED[w, T, 3]
    _, whole = restate([recs], 4, w, T)
    if w == 8:
        assert len(a[1]) < len(whole), (len(a[1]), len(whole))
        est = [e[4] for e in a[2]]
        print("estimates at ranks 15..16: %s" % est[-2:])
    else:
        assert a[1] == whole


def tie_order(be):
    """w = 2^8: several candidates share an estimate; within it the order is the key's."""
    pods, recs = planted()
    cms, cand = restate([recs], 4, 8, 300)
    top = topk(cms, cand, len(cand))
    est = [e[4] for e in top]
    ties = [k for k in range(1, len(top)) if est[k] == est[k - 1]]
    assert ties, "the workload has no tie"
    g = be.engine(pods, 4, 8, 0)
    try:
        g.set_heavy_hitters(300, 0)
        keep = be.submit(g, recs)
        for k in sorted({ties[0], ties[0] + 1, ties[-1], ties[-1] + 1}):  # k cuts a run of equal estimates
            assert rows(g.heavy_hitters(k)) == top[:k], k
        del keep
    finally:
        g.close()


# ---- unaligned columns, ragged n ------------------------------------------------------------
RAGGED = ["1", "3", "4cu-1", "4cu+1", "1024cu+5"]


def ragged(be, which: str, unaligned: bool):
    """T = 1: every record's key is a candidate.  Below 4 * CUs records the last workgroups'
    chunks start at or past n; n % 4 != 0 splits the last chunk into vector body and scalar
    tail; unaligned columns take the scalar-load kernel throughout."""
    cu = be.cus
    n = {"1": 1, "3": 3, "4cu-1": 4 * cu - 1, "4cu+1": 4 * cu + 1, "1024cu+5": 1024 * cu + 5}[which]
    pods, recs = K.inputs(100, max(n, 1024 * 256 + 5), 9)
    part = take(recs, slice(0, n))
    if n < 8:
        part.src_ip = pods.ips[:n].copy()
    lg = max(4, math.ceil(math.log2(2 * n)))
    _, cand, _ = run(be, pods, [part], 4, 12, 10, 1, lg, unaligned=unaligned)
    assert len(cand) == len(np.unique(keys_of(part), axis=0))


# ---- depths -----------------------------------------------------------------------------------
DEPTHS = [1, 3, 9, 16]


def depths(be, d: int):
    """The candidate kernel's own depth loop; the scatter changes kernel at 9.  No HLL: the
    count-min lists are the only deferred ones."""
    pods, recs = planted()
    run(be, pods, thirds(recs), d, 10, 0, 300, 0)


# ---- one key on many lanes --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hot_inputs():
    pods, base = K.inputs(100, 1 << 18, 22)
    recs = W.Records(base.src_ip.copy(), base.dst_ip.copy(), base.bytes, base.meta.copy(), base.ports.copy(),
                     base.dns_id)
    hot = np.random.default_rng(23).random(len(recs)) < 0.5
    for col in (recs.src_ip, recs.dst_ip, recs.meta, recs.ports):
        col[hot] = col[0]
    return pods, recs, int(hot.sum()) + (0 if hot[0] else 1)


def one_key_many_lanes(be):
    """Half of 2^18 records one 5-tuple, mixed at random over every workgroup: the key is
    first claimed by every workgroup at once, and a 16-slot table must hold it once."""
    pods, recs, n_hot = hot_inputs()
    cms, cand = restate([recs], 4, 12, 1000)
    assert len(cand) <= 8
    hot = tuple(int(x) for x in keys_of(recs)[0])
    assert hot in cand
    _, _, top = run(be, pods, [recs], 4, 12, 10, 1000, 4)
    assert [e[:4] for e in top].count(hot) == 1
    assert top[0][:4] == hot and top[0][4] == int(estimate(cms, [hot])[0]) >= n_hot


# ---- a full table -----------------------------------------------------------------------------
def table_full(be):
    pods, recs = planted()
    cms, cand = restate([recs], 4, 8, 300)
    assert len(cand) > 16
    g = be.engine(pods, 4, 8, 10)
    try:
        g.set_heavy_hitters(300, 4)
        keep = be.submit(g, recs)
        got = candidates(g)
        info = g.hh_info()
        print("%d restated, %d stored, %d refused" % (len(cand), len(got), info["dropped"]))
        assert info["dropped"] > 0 and info["candidates"] == len(got)
        assert got <= cand and 8 <= len(got) <= 16
        assert rows(g.heavy_hitters(100)) == topk(cms, got, 100)  # every estimate exact
        K.verify(g, pods, [recs], 4, 8, 10)
        del keep
        g.reset()
        assert len(g.hh_candidates()) == 0 and len(g.heavy_hitters(5)) == 0
        assert g.hh_info() == {"candidates": 0, "dropped": 0, "min_count": 300, "capacity_log2": 4}
    finally:
        g.close()


# ---- off, on, off -----------------------------------------------------------------------------
def raises(code, fn, *a):
    with pytest.raises(GpuAggError) as e:
        fn(*a)
    assert e.value.code == code, e.value


def off_and_on(be):
    pods, recs = planted()
    parts = thirds(recs)
    g = be.engine(pods, 4, 12, 10)
    try:
        raises(_abi.ESTATE, g.heavy_hitters, 4)
        raises(_abi.ESTATE, g.hh_candidates)
        raises(_abi.ESTATE, g.hh_add_candidates, np.zeros((1, 4), np.uint32))
        assert g.hh_info()["min_count"] == 0
        raises(_abi.EINVAL, g.set_heavy_hitters, 300, 3)
        raises(_abi.EINVAL, g.set_heavy_hitters, 300, 25)
        keep = [be.submit(g, parts[0])]
        g.set_heavy_hitters(300, 0)  # mid-stream: only later submits admit
        keep += [be.submit(g, r) for r in parts[1:]]
        cms, cand = restate(parts, 4, 12, 300, test_from=1)
        assert cand
        check(g, pods, parts, 4, 12, 10, cms, cand)
        g.set_heavy_hitters(600, 0)  # another threshold: the candidates start over
        assert g.hh_info() == {"candidates": 0, "dropped": 0, "min_count": 600, "capacity_log2": 16}
        g.set_heavy_hitters(0, 0)
        raises(_abi.ESTATE, g.heavy_hitters, 4)
        raises(_abi.ESTATE, g.hh_candidates)
        keep.append(be.submit(g, parts[0]))  # and the submit path runs without it again
        K.verify(g, pods, parts + [parts[0]], 4, 12, 10)
        del keep
    finally:
        g.close()
    g = be.engine(pods, 0, 0, 10)
    try:
        raises(_abi.ESTATE, g.set_heavy_hitters, 300, 0)
    finally:
        g.close()


# ---- host keys, merge -------------------------------------------------------------------------
def add_candidates(be):
    """Keys no record has (protocol 200) come back with their collision count."""
    pods, recs = planted()
    cms, cand = restate([recs], 4, 8, 300)
    absent = np.array(sorted(cand)[:5], np.uint32)
    absent[:, 3] = 200
    g = be.engine(pods, 4, 8, 10)
    try:
        g.set_heavy_hitters(300, 0)
        keep = be.submit(g, recs)
        g.hh_add_candidates(absent)
        g.hh_add_candidates(absent)  # twice: still once each
        g.hh_add_candidates(np.array(sorted(cand)[:3], np.uint32))  # already there
        both = cand | set(tuple(int(x) for x in k) for k in absent)
        assert len(both) == len(cand) + 5
        check(g, pods, [recs], 4, 8, 10, cms, both)
        del keep
    finally:
        g.close()


def merge(be):
    """Two engines on one device, each fed half the flows by 5-tuple parity: the merged
    candidates are the union, the estimates come from the summed rows."""
    pods, recs = planted()
    key = keys_of(recs)
    odd = ((key[:, 0] ^ key[:, 1] ^ key[:, 2] ^ key[:, 3]) & 1).astype(bool)
    halves = [take(recs, np.flatnonzero(~odd)), take(recs, np.flatnonzero(odd))]
    T, w = 300, 8
    (cms0, cand0), (cms1, cand1) = restate([halves[0]], 4, w, T), restate([halves[1]], 4, w, T)
    assert cand0 and cand1 and not cand0 & cand1
    gs = [be.engine(pods, 4, w, 10), be.engine(pods, 4, w, 10)]
    try:
        gs[0].set_heavy_hitters(T, 0)
        gs[1].set_heavy_hitters(T + 1, 0)
        keep = [be.submit(g, r) for g, r in zip(gs, halves)]
        before = [(candidates(g), g.cms_array()) for g in gs]
        assert before[0][0] == cand0
        raises(_abi.EINVAL, gs[0].merge_from, [gs[1]])  # unequal min_count: nothing moves
        for g, (c, rows_) in zip(gs, before):
            assert candidates(g) == c and np.array_equal(g.cms_array(), rows_)
        gs[1].set_heavy_hitters(T, 0)
        gs[1].reset()
        keep.append(be.submit(gs[1], halves[1]))
        assert candidates(gs[1]) == cand1
        gs[0].merge_from([gs[1]])
        check(gs[0], pods, halves, 4, w, 10, cms0 + cms1, cand0 | cand1)
        assert gs[1].hh_info() == {"candidates": 0, "dropped": 0, "min_count": T, "capacity_log2": 16}
        del keep
    finally:
        for g in gs:
            g.close()


# ---- distinct peers of every pod ------------------------------------------------------------
HLL_P = [4, 14, 18]
FEW, MANY = 7, 9


@functools.lru_cache(maxsize=None)
def hll_workload():
    """The workload of sketch_cases.hll_estimates: pod FEW has seen three destinations, pod
    MANY thousands."""
    pods, base = K.inputs(64, 100_000, 12)
    recs = W.Records(base.src_ip.copy(), base.dst_ip.copy(), base.bytes, base.meta, base.ports, base.dns_id)
    few_ips = np.array(pods.endpoints[FEW].ips, np.uint32)
    recs.src_ip[np.isin(recs.src_ip, few_ips)] = pods.endpoints[MANY].ips[0]
    recs.src_ip[:3] = few_ips[0]
    recs.dst_ip[:3] = np.array([W.ip_le(100, 70, 0, 1), W.ip_le(100, 70, 0, 2), W.ip_le(100, 70, 0, 3)], np.uint32)
    recs.src_ip[1000:6000] = pods.endpoints[MANY].ips[0]
    recs.dst_ip[1000:6000] = np.random.default_rng(13).integers(1, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32)
    return pods, recs


def hll_all(be, p: int):
    """hll_estimates()[s] against oracle.sketch.hll_estimate and gpuagg_hll_estimate, within
    sketch_cases.HLL_EST_TOL (its derivation covers the exact integer sums as well: they
    round once where the others round per term)."""
    pods, recs = hll_workload()
    np_ = len(pods.endpoints)
    g = be.engine(pods, 4, 12, p)
    try:
        keep = be.submit(g, recs)
        est = g.hll_estimates()  # before any other read: folds what is pending itself
        _, want_h = K.verify(g, pods, [recs], 4, 12, p)
        del keep
        assert est.dtype == np.float64 and len(est) == g.hll_array().shape[0] >= np_
        g.sketch_refresh()
        for s in range(np_):
            want = S.hll_estimate(want_h[s])
            assert abs(est[s] - want) <= K.HLL_EST_TOL * want, (s, est[s], want)
            one = g.hll_estimate(s)
            assert abs(est[s] - one) <= K.HLL_EST_TOL * one, (s, est[s], one)
        assert est[MANY] > 2000
        assert (est[np_:] == 0.0).all()
        empty = np.flatnonzero(~want_h.any(axis=1))
        assert (est[empty] == 0.0).all()
        if p == 4:
            zeros = int((want_h[FEW] == 0).sum())
            assert 13 <= zeros <= 15
            lc = 16 * math.log(16 / zeros)
            assert abs(est[FEW] - lc) <= K.HLL_EST_TOL * lc
            assert not (want_h[MANY] == 0).any() and est[MANY] > 2.5 * 16
        assert np.array_equal(g.hll_estimates(), est)  # reading changes nothing
    finally:
        g.close()
    g = be.engine(pods, 4, 12, 0)
    try:
        raises(_abi.ESTATE, g.hll_estimates)
    finally:
        g.close()


def hll_growth(be):
    """The slot table grows between two submits: the returned length follows the rows."""
    pods = W.make_pods(1_100, seed=641)
    few = W.Pods(pods.endpoints[:100], pods.ips, pods.ip_owner)
    recs = W.gen_records(60_000, pods, seed=642)
    half = len(recs) // 2
    g = be.engine(few, 4, 12, 8, max_slots=2048, max_ips=4096)
    try:
        keep = [be.submit(g, take(recs, slice(0, half)))]
        n0 = len(g.hll_estimates())
        assert n0 == g.hll_array().shape[0]
        g.load_endpoints(pods.endpoints[100:], version=2)
        keep.append(be.submit(g, take(recs, slice(half, None))))
        est = g.hll_estimates()
        regs = g.hll_array()
        assert len(est) == regs.shape[0] > n0 and regs.shape[0] >= 1_100
        assert regs[100:1_100].any()
        for s in range(regs.shape[0]):
            want = S.hll_estimate(regs[s])
            assert abs(est[s] - want) <= K.HLL_EST_TOL * want, (s, est[s], want)
        del keep
    finally:
        g.close()
