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
The case functions print the candidate counts they see.

The table's own edges (second half of the module) need keys chosen by where they land: pool()
draws 2^21 keys and the numpy restatement of the readout's hash slices (home, tag, LDS-set home)
picks 16 keys of one home for a 16-slot table, pairs with one tag and one home, six keys of one
LDS-set home.  There each chosen key occurs TABLE_T = 32 times in one submit among filler keys
that occur once, at 2^16 columns; the restatement decides what is admitted, and every case
asserts that this is exactly the chosen set."""

from __future__ import annotations

import ctypes as C
import functools
import math
import subprocess
import time

import numpy as np
import pytest

from oracle import sketch as S
from retina_amd import _abi
from retina_amd import workloads as W
from retina_amd.engine import GpuAggError

from . import host_programs
from . import sketch_cases as K
from .growth_inputs import take

PER_BATCH, DIRECT = _abi.FLAG_FOLD_PER_BATCH, _abi.FLAG_DIRECT_SKETCH
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


def check(g, pods, parts, d, w, p, cms, cand, dropped=0, want=None):
    """The four assertions of every case (module docstring).  want: the restated (rows,
    registers) where the parts alone do not give them (sketch_ops_cases.py: another slot map
    for a part, rows zeroed in between)."""
    got = candidates(g)
    assert got == cand, "candidates: %d missing, %d unexpected (of %d restated)" % (
        len(cand - got), len(got - cand), len(cand))
    for k in (1, 16, len(cand) + 5):
        assert rows(g.heavy_hitters(k)) == topk(cms, cand, k), "top-%d" % k
    info = g.hh_info()
    assert info["candidates"] == len(cand) and info["dropped"] == dropped, info
    if want is None:
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


# ---- the readout's hash slices and a pool of keys to choose from by them -------------------------
# gpuagg_launch.h (kHhHomeShift, kHhTagShift / kHhTagBits, kHhLdsShift / kHhLdsLog2) restated;
# test_hh_cpu.py::test_hash_slices pins the restatement against tests/hh_hash_test.cpp.  The
# tag's bits 15..25 are the LDS-set home: keys that share a tag share that home too.
HOME_SHIFT, TAG_SHIFT, TAG_BITS, LDS_SHIFT, LDS_LOG2, LDS_PROBE = 13, 35, 29, 50, 11, 4
assert TAG_SHIFT <= LDS_SHIFT and LDS_SHIFT + LDS_LOG2 <= TAG_SHIFT + TAG_BITS


def cms_base(keys) -> np.ndarray:
    k = np.asarray(keys, np.uint32).reshape(-1, 4).astype(S.U64)
    return S.fmix64((k[:, 0] | (k[:, 1] << S.U64(32))) ^ S.fmix64((k[:, 2] | (k[:, 3] << S.U64(32))) ^ S.CMS_SEED))


def home(base, lg: int) -> np.ndarray:
    """The home slot in a table of 2^lg slots (lg = 32: what hh_hash_test prints)."""
    return ((base >> S.U64(HOME_SHIFT)) & S.U64((1 << lg) - 1)).astype(np.int64)


def tag(base) -> np.ndarray:
    return ((base >> S.U64(TAG_SHIFT)) & S.U64((1 << TAG_BITS) - 1)).astype(np.int64)


def lds_home(base) -> np.ndarray:
    return ((base >> S.U64(LDS_SHIFT)) & S.U64((1 << LDS_LOG2) - 1)).astype(np.int64)


def host_slices(keys) -> np.ndarray:
    """uint64 [n, 4]: (cms_base, base >> kHhHomeShift as u32, tag, LDS-set home) of uint32 [n, 4]
    keys by tests/hh_hash_test.cpp."""
    exe = host_programs.build("hh_hash_test")
    text = "".join("%d %d %d %d\n" % tuple(k) for k in np.asarray(keys, np.uint32).reshape(-1, 4).tolist())
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    got = np.array([[int(x) for x in ln.split()] for ln in out.splitlines()], np.uint64).reshape(-1, 4)
    assert len(got) == len(keys)
    return got


POOL_LOG2 = 21


@functools.lru_cache(maxsize=None)
def pool():
    """(keys uint32 [2^21, 4], their cms_base): uniform 32-bit words, protocol 6 or 17."""
    rng, n = np.random.default_rng(77), 1 << POOL_LOG2
    src, dst, ports = rng.integers(0, 2**32, n), rng.integers(0, 2**32, n), rng.integers(0, 2**32, n)
    proto = np.where(rng.random(n) < 0.5, 6, 17)
    keys = np.stack([src, dst, ports, proto], 1).astype(np.uint32)
    return keys, cms_base(keys)


def groups_of(v: np.ndarray, least: int = 2):
    """The index sets (ascending, ordered by their first index) of at least `least` equal values."""
    order = np.argsort(v, kind="stable")
    sv = v[order]
    cut = np.flatnonzero(sv[1:] != sv[:-1]) + 1
    runs = [r for r in np.split(order, cut) if len(r) >= least]
    return sorted(runs, key=lambda r: int(r[0]))


@functools.lru_cache(maxsize=None)
def twins(lg: int):
    """Pool keys that share the tag and the home of a 2^lg-slot table; lg = 0: the tag alone."""
    _, base = pool()
    return groups_of((tag(base) << lg) | home(base, lg))


@functools.lru_cache(maxsize=None)
def table_pods():
    return W.make_pods(100, seed=677)


def key_records(keys) -> W.Records:
    """One forwarded record per key row (the pool's sources are no pod's: no HLL update)."""
    k = np.asarray(keys, np.uint32).reshape(-1, 4)
    n, u = len(k), np.uint32
    return W.Records(k[:, 0].copy(), k[:, 1].copy(), np.full(n, 64, u), W.pack_meta(k[:, 3], W.V_FWD, 1).astype(u),
                     k[:, 2].copy(), np.zeros(n, u))


def filler(n: int, chosen) -> np.ndarray:
    """n pool keys, none of them among the pool indices `chosen`: each occurs once."""
    keys, _ = pool()
    at = np.setdiff1d(np.arange(n + len(chosen)), np.asarray(chosen))[:n]
    assert len(at) == n <= len(keys)
    return keys[at]


def as_set(keys):
    return set(tuple(int(x) for x in k) for k in np.asarray(keys).reshape(-1, 4))


TABLE_W, TABLE_T = 16, 32  # the table cases: each chosen key TABLE_T times in one submit


def front_loaded(be, chosen_at, layout):
    """1024 records per workgroup (one workgroup per CU, chunk = ceil(n / CUs)); positions
    layout[i] < 1024, all inside the first workgroup's chunk, hold pool key chosen_at[i], every
    other position a filler key of its own."""
    keys, _ = pool()
    n = 1024 * be.cus
    assert n <= len(keys) and len(chosen_at) == len(layout) and max(layout) < 1024
    rec = np.empty((n, 4), np.uint32)
    free = np.ones(n, bool)
    free[layout] = False
    rec[layout] = keys[chosen_at]
    rec[free] = filler(int(free.sum()), np.unique(chosen_at))
    return key_records(rec)


def table_engine(be, lg, flags=0, w=TABLE_W, T=TABLE_T):
    g = be.engine(table_pods(), 4, w, 0, flags)
    try:
        g.set_heavy_hitters(T, lg)
    except BaseException:
        g.close()
        raise
    return g


def heavy_none(g):
    """k = 0: nothing, and no out pointer is needed."""
    n = C.c_size_t(7)
    assert g.lib.gpuagg_heavy_hitters(g.h, None, 0, C.byref(n)) == _abi.OK and n.value == 0


# ---- one home, a table filled exactly ---------------------------------------------------------
CHAIN_HOME = 13  # of 16 slots: the chain runs 13, 14, 15, 0, ... 12


def same_home_chain(be, through: str):
    """capacity_log2 = 4 and 16 keys whose home is slot 13: every probe chain wraps the table,
    the table ends up filled exactly, the last key probes all 16 slots.  through "add":
    hh_add_candidates (one call, then the same again); "records": each key 32 times in one
    submit, mixed over every workgroup.  Three more keys of that home are each refused once."""
    keys, base = pool()
    at = np.flatnonzero(home(base[:8192], 4) == CHAIN_HOME)[:19]
    assert len(at) == 19 and CHAIN_HOME != 0
    chosen, extra = keys[at[:16]], keys[at[16:]]
    fill = filler(20_000, at)
    if through == "records":
        mixed = np.concatenate([np.repeat(chosen, TABLE_T, axis=0), fill])
        recs = key_records(mixed[np.random.default_rng(78).permutation(len(mixed))])
    else:
        recs = key_records(fill)
    pods, want = table_pods(), as_set(chosen)
    cms, cand = restate([recs], 4, TABLE_W, TABLE_T)
    assert cand == (want if through == "records" else set())
    g = table_engine(be, 4)
    try:
        keep = be.submit(g, recs)
        if through == "add":
            g.hh_add_candidates(chosen)
            g.hh_add_candidates(chosen)
        check(g, pods, [recs], 4, TABLE_W, 0, cms, want)
        del keep
        g.hh_add_candidates(extra)
        check(g, pods, [recs], 4, TABLE_W, 0, cms, want, dropped=3)
        g.hh_add_candidates(chosen)  # all there: found, not refused
        check(g, pods, [recs], 4, TABLE_W, 0, cms, want, dropped=3)
        heavy_none(g)
        for k in (1, 16, 40):
            assert rows(g.heavy_hitters(k)) == topk(cms, want, k), k
    finally:
        g.close()


# ---- two keys, one tag, one home --------------------------------------------------------------
TWINS = {4: 4, 8: 8}  # capacity_log2: pairs


def tag_twins(be, lg: int, through: str):
    """Pairs of keys with equal tag and equal home (so equal LDS-set home): a probe that meets
    the twin's slot reads a full tag that matches and must compare the key -- and, while the
    twin is being written, wait at its pending tag and then probe on.  "add": every pair side
    by side in one hh_add_candidates call (a wave per key); "records": the first workgroup's
    chunk holds every pair's 2 * 32 records, pair i alternating its two keys record by record
    (i odd) or four records at a time (i even: a lane's four records one key, neighbouring
    lanes the twin), so both keys pass in the same wave."""
    keys, _ = pool()
    pairs = [r[:2] for r in twins(lg)[:TWINS[lg]]]
    print("2^%d slots: %d groups of keys with one tag and one home" % (lg, len(twins(lg))))
    assert len(pairs) == TWINS[lg], "the pool has %d twin groups for 2^%d slots" % (len(twins(lg)), lg)
    chosen_at = np.concatenate(pairs)
    chosen, pods = keys[chosen_at], table_pods()
    if through == "records":
        at, layout = [], []
        for i, (a, b) in enumerate(pairs):
            unit = 4 if i % 2 == 0 else 1
            for j in range(2 * TABLE_T):
                at.append(a if (j // unit) % 2 == 0 else b)
                layout.append(2 * TABLE_T * i + j)
        recs = front_loaded(be, np.array(at), np.array(layout))
    else:
        recs = key_records(filler(20_000, chosen_at))
    cms, cand = restate([recs], 4, TABLE_W, TABLE_T)
    want = as_set(chosen)
    assert len(want) == 2 * len(pairs) and cand == (want if through == "records" else set())
    g = table_engine(be, lg)
    try:
        keep = be.submit(g, recs)
        if through == "add":
            g.hh_add_candidates(chosen)
        check(g, pods, [recs], 4, TABLE_W, 0, cms, want)
        del keep
    finally:
        g.close()


# ---- the per-workgroup LDS set ------------------------------------------------------------------
def lds_six(be):
    """Six keys with one LDS-set home in one workgroup's chunk, each 32 times at the even
    positions below 384 (two waves' records): the set tries LDS_PROBE = 4 entries, so two of
    the keys are never remembered and go to the table every time they pass -- where they are
    found.  Exactly six candidates, nothing refused."""
    keys, base = pool()
    group = groups_of(lds_home(base[:100_000]), 6)
    print("LDS-set homes with >= 6 of the first 100,000 keys: %d, the fullest has %d" % (
        len(group), max(len(r) for r in group)))
    six = group[0][:6]
    assert len(six) == 6 > LDS_PROBE and len(as_set(keys[six])) == 6
    layout = 2 * np.arange(6 * TABLE_T)
    recs = front_loaded(be, six[np.arange(6 * TABLE_T) % 6], layout)
    cms, cand = restate([recs], 4, TABLE_W, TABLE_T)
    assert cand == as_set(keys[six])
    g = table_engine(be, 0)
    try:
        keep = be.submit(g, recs)
        check(g, table_pods(), [recs], 4, TABLE_W, 0, cms, cand)
        del keep
    finally:
        g.close()


def sorted_rows(keys) -> np.ndarray:
    k = np.asarray(keys, np.uint32).reshape(-1, 4)
    return k[np.lexsort((k[:, 3], k[:, 2], k[:, 1], k[:, 0]))]


def lds_overflow(be):
    """4,096 distinct keys per workgroup, T = 1: every one passes, twice the 2^11 entries of
    the LDS set; the same records again find every key in the table (through the set or
    not).  About a million candidates in 2^21 slots: compared as sorted rows, the top-k in
    numpy."""
    keys, _ = pool()
    n = 4096 * be.cus
    assert n <= len(keys) // 2, "more than 256 CUs: the pool is too small for this case"
    rec = keys[:n]
    want = sorted_rows(rec)
    assert (want[1:] != want[:-1]).any(axis=1).all(), "the pool's keys are distinct"
    recs, pods = key_records(rec), table_pods()
    cms = np.zeros((4, 1 << TABLE_W), np.uint32)
    g = table_engine(be, 21, T=1)
    try:
        keep = []
        for submit in range(2):
            keep.append(be.submit(g, recs))
            S.cms_update(cms, rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3])
            got = g.hh_candidates()
            assert got.shape == want.shape and np.array_equal(sorted_rows(got), want), submit
            info = g.hh_info()
            assert info["candidates"] == n and info["dropped"] == 0, (submit, info)
        est = estimate(cms, rec)
        order = np.lexsort((rec[:, 3], rec[:, 2], rec[:, 1], rec[:, 0], -est))[:16]
        top = [tuple(int(x) for x in rec[i]) + (int(est[i]),) for i in order]
        for k in (1, 16):
            assert rows(g.heavy_hitters(k)) == top[:k], k
        K.verify(g, pods, [recs, recs], 4, TABLE_W, 0, (cms, None))
        del keep
    finally:
        g.close()


# ---- estimates of zero ----------------------------------------------------------------------------
def zero_estimates(be):
    """20 keys added before any record: every estimate is 0, so a candidate's sort key has the
    high word 2^32 - 1 - 0 -- the high word of a free slot's all-ones sort key.  The ranking
    must still hand over exactly the candidates, in key order; then records arrive."""
    pods, recs = planted()
    cms, cand = restate([recs], 4, 12, 300)
    absent = np.array(sorted(cand)[:20], np.uint32)
    absent[:, 3] = 200
    assert len(as_set(absent)) == 20 and not as_set(absent) & cand
    g = be.engine(pods, 4, 12, 10)
    try:
        g.set_heavy_hitters(300, 0)
        g.hh_add_candidates(absent)
        zero = [k + (0,) for k in sorted(as_set(absent))]
        for k in (1, 7, 20, 25):
            assert rows(g.heavy_hitters(k)) == zero[:k], k
        heavy_none(g)
        assert g.hh_info()["candidates"] == 20 and candidates(g) == as_set(absent)
        keep = be.submit(g, recs)
        check(g, pods, [recs], 4, 12, 10, cms, cand | as_set(absent))
        del keep
    finally:
        g.close()


# ---- the largest table, direct rows, capacity reports -----------------------------------------
def largest_table(be):
    """capacity_log2 = 24: 2^24 slots of 20 bytes and 16 bytes per slot for the ranking."""
    pods, recs = planted()
    t0 = time.perf_counter()
    _, cand, _ = run(be, pods, [recs], 4, 12, 10, 300, 24)
    print("capacity_log2 = 24: %.2f s" % (time.perf_counter() - t0))
    assert len(cand) == RESTATED[12, 300, 1] == 37


def direct_rows(be):
    """FLAG_DIRECT_SKETCH: the count-min rows are updated by atomics in the scatter kernel, no
    list waits and the candidate pass has nothing to fold first; as the deferred engine."""
    pods, recs = planted()
    parts = thirds(recs)
    a = run(be, pods, parts, 4, 12, 10, 300, 0)
    b = run(be, pods, parts, 4, 12, 10, 300, 0, DIRECT)
    assert a[1] == b[1] and a[2] == b[2] and len(a[1]) == RESTATED[12, 300, 3]


def capacity_reports(be):
    """Room for one entry less than there are: ECAPACITY, and n is what is needed."""
    pods, recs = planted()
    _, cand = restate([recs], 4, 12, 300)
    g = be.engine(pods, 4, 12, 10)
    try:
        g.set_heavy_hitters(300, 0)
        keep = be.submit(g, recs)
        n = C.c_size_t()
        out = np.zeros((len(cand), 4), np.uint32)
        assert g.lib.gpuagg_hh_candidates(g.h, out.ctypes.data_as(_abi.u32p), len(cand) - 1, C.byref(n)) == _abi.ECAPACITY
        assert n.value == len(cand) and not out.any()
        assert g.lib.gpuagg_hh_candidates(g.h, out.ctypes.data_as(_abi.u32p), len(cand), C.byref(n)) == _abi.OK
        assert n.value == len(cand) and as_set(out) == cand
        del keep
        rows_ = g.hll_array().shape[0]
        est = np.zeros(rows_, np.float64)
        dp = est.ctypes.data_as(C.POINTER(C.c_double))
        assert g.lib.gpuagg_hll_estimate_all(g.h, dp, rows_ - 1, C.byref(n)) == _abi.ECAPACITY
        assert n.value == rows_ and not est.any()
        assert g.lib.gpuagg_hll_estimate_all(g.h, dp, rows_, C.byref(n)) == _abi.OK
        assert n.value == rows_ and np.array_equal(est, g.hll_estimates()) and est.any()
    finally:
        g.close()


# ---- distinct peers: every precision, a row count that is no multiple of 4 ---------------------
HLL_SWEEP = list(range(4, 19))
SWEEP_ROWS = 50


def hll_sweep(be, p: int):
    """max_slots = 50 caps the rows at 50 (64 otherwise): up to p = 12 the last workgroup of the
    wave-per-pod kernel has two waves past the rows, from 13 on a workgroup reduces a pod."""
    pods, recs = K.inputs(40, 30_000, 31)
    np_ = len(pods.endpoints)
    assert np_ <= SWEEP_ROWS and SWEEP_ROWS % 4 != 0
    g = be.engine(pods, 4, 12, p, max_slots=SWEEP_ROWS)
    try:
        keep = be.submit(g, recs)
        est = g.hll_estimates()
        _, want_h = K.verify(g, pods, [recs], 4, 12, p)
        del keep
        assert len(est) == g.hll_array().shape[0] == SWEEP_ROWS
        g.sketch_refresh()
        for s in range(np_):
            want = S.hll_estimate(want_h[s])
            assert abs(est[s] - want) <= K.HLL_EST_TOL * want, (s, est[s], want)
            one = g.hll_estimate(s)
            assert abs(est[s] - one) <= K.HLL_EST_TOL * one, (s, est[s], one)
        assert est[:np_].any() and (est[np_:] == 0.0).all()
    finally:
        g.close()


# ---- ranks above 32 -----------------------------------------------------------------------------
# p: (dst_ip column value, rank of fmix64(dst ^ HLL_SEED) at that precision), from a search over
# all 2^32 destinations; none reaches 33 at p = 12, 13, 14, 16, 17.
HIGH_RANK = {4: (2445276856, 33), 5: (489467923, 35), 6: (489467923, 34), 7: (3296042774, 34),
             8: (1898538810, 36), 9: (1898538810, 35), 10: (1898538810, 34), 11: (3352010515, 33),
             15: (2624332809, 33), 18: (355453830, 36)}
HIGH_POD = 5


@functools.lru_cache(maxsize=2)
def high_rank_records(p: int):
    """4,000 ordinary records, then 3 * 2^p from pod HIGH_POD towards random destinations --
    enough for the estimator to leave linear counting -- eight of them towards HIGH_RANK[p]."""
    pods, base = K.inputs(40, 4_000, 32)
    n, u = 3 << p, np.uint32
    hot = np.random.default_rng(33).integers(1, 1 << 32, n, dtype=np.uint64).astype(u)
    hot[np.arange(8) * (n // 8)] = HIGH_RANK[p][0]

    def col(a, fill):
        return np.concatenate([a, np.full(n, fill, u)]).astype(u)
    recs = W.Records(col(base.src_ip, pods.endpoints[HIGH_POD].ips[0]), np.concatenate([base.dst_ip, hot]).astype(u),
                     col(base.bytes, 64), col(base.meta, base.meta[0]), col(base.ports, base.ports[0]),
                     col(base.dns_id, 0))
    return pods, recs


def hll_high_ranks(be, p: int):
    """One pod sends to a destination whose rank is above 32, among ordinary records, under
    deferred lists, per-batch folds and direct updates: the registers bit-exact (the rank
    survives the list entry's packing and the fold's maximum), and the readout takes
    2^-r from the other of its two integer sums (r <= 32: 2^(32 - r), else 2^(64 - r)).  A
    rank above 32 counted on the r <= 32 side would shift by a negative amount -- 2^31 or
    more added to a sum whose other terms are at most 2^31 each -- and move the estimate by
    orders of magnitude.  What this cannot show is the high sum being dropped altogether:
    the one term 2^-33 or less, against a sum of at least 2^-1 (the pod's other registers),
    changes the estimate by less than HLL_EST_TOL, and the tolerance is not tightened for it."""
    dst, rank = HIGH_RANK[p]
    pods, recs = high_rank_records(p)
    want = K.expected(pods, [recs], 4, 12, p)
    assert int(want[1][HIGH_POD].max()) == rank >= 33
    # the raw estimate, not linear counting (which reads the zero registers alone and would
    # hide the sums): the pod has sent to three destinations per register
    assert S.hll_estimate(want[1][HIGH_POD]) > 2.5 * (1 << p)
    for flags in (0, PER_BATCH, DIRECT):
        g = be.engine(pods, 4, 12, p, flags)
        try:
            keep = be.submit(g, recs)
            print("p=%d flags=%d: %s" % (p, flags, g.sketch_kernel_name() or "(host)"))
            est = g.hll_estimates()
            K.verify(g, pods, [recs], 4, 12, p, want)
            del keep
            assert int(g.hll_array()[HIGH_POD].max()) == rank
            g.sketch_refresh()
            exact = S.hll_estimate(want[1][HIGH_POD])
            assert abs(est[HIGH_POD] - exact) <= K.HLL_EST_TOL * exact, (flags, est[HIGH_POD], exact)
            one = g.hll_estimate(HIGH_POD)
            assert abs(one - exact) <= K.HLL_EST_TOL * exact, (flags, one, exact)
        finally:
            g.close()
