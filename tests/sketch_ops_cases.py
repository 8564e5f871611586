"""State operations while the sketches' deferred scatter lists are still waiting, written once
and run on both backends: test_sketch_ops_cpu.py (GPUAGG_FLAG_CPU_BACKEND, host-fed) and
test_gpu_sketch_ops.py (gfx950, device-resident submits).

Every case: an engine with count-min (d = 4, w = 2^10), HLL (p = 8, 100 pods) and heavy hitters
(min_count 60); part 1 (20,000 records) submitted unsynced and not read; the operation; part 2
unsynced; then the count-min rows and the HLL registers bit-exact against oracle/sketch.py
(sketch_cases.verify) and the candidates, the top-k and hh_info against the restated candidate
rule (hh_cases.check).  Under flags 0 the records of part 1 are still in the deferred lists
(sk_pend) when the operation runs -- it has to fold them first, or discard them, as its meaning
demands; FLAG_FOLD_PER_BATCH folds in every launch and FLAG_DIRECT_SKETCH has no lists: all
three must agree with the one restatement.

The records: the planted workload of hh_cases (48 flows of 40 + 25 j records among 60,000),
in three slices of 20,000.  At 2^10 columns a part puts about 20 records on every column, so
min_count = 60 admits the planted flows with about 60 records or more in a part and a few
keys that collide with them: tens of candidates, different for every part (asserted)."""

from __future__ import annotations

import functools
import os
import types

import numpy as np

from oracle import sketch as S
from retina_amd import workloads as W

from . import hh_cases as H
from . import sketch_cases as K
from .growth_inputs import take

D, WLOG2, P, T = 4, 10, 8, 60
FLAGS = {"deferred": 0, "per-batch": K.PER_BATCH, "direct": K.DIRECT}
OTHER_SPEC = [{"metric_name": "forward_count", "source_labels": ["namespace"]}]
SAME_SPEC = [{"metric_name": "forward_count", "source_labels": ["podname", "namespace"]}]
assert sorted(SAME_SPEC[0]["source_labels"]) == sorted(K.SPEC[0]["source_labels"]) != SAME_SPEC[0]["source_labels"]


def copy_of(r: W.Records) -> W.Records:
    return W.Records(r.src_ip.copy(), r.dst_ip.copy(), r.bytes.copy(), r.meta.copy(), r.ports.copy(), r.dns_id.copy())


@functools.lru_cache(maxsize=None)
def parts():
    """(pods, part 1, part 2, part 3): part 3 is what a second engine holds in the merge."""
    pods, recs = H.planted()
    assert len(pods.endpoints) == 100 and len(recs) == 60_000
    return (pods,) + tuple(copy_of(take(recs, slice(a, a + 20_000))) for a in (0, 20_000, 40_000))


def slot_map(ips_by_slot):
    """What sketch_cases.src_slots needs of the pods: endpoints[s].ips."""
    return types.SimpleNamespace(endpoints=[types.SimpleNamespace(ips=list(ips)) for ips in ips_by_slot])


def registers(n_slots: int, *steps) -> np.ndarray:
    """HLL registers after steps of (slot map, records)."""
    h = np.zeros((n_slots, 1 << P), np.uint8)
    for pods, r in steps:
        S.hll_update(h, K.src_slots(pods, r.src_ip), r.dst_ip, P)
    return h


def engine(be, pods, flags, **kw):
    g = be.engine(pods, D, WLOG2, P, flags, **kw)
    try:
        g.set_heavy_hitters(T, 0)
    except BaseException:
        g.close()
        raise
    return g


INFO = {"min_count": T, "capacity_log2": 16}


def finish(g, pods, done, cms, cand, want_h=None):
    """The closing assertions; want_h: registers that the parts under one slot map do not give."""
    print("flags=%d: %s; %d candidates" % (g.cfg.flags, g.sketch_kernel_name() or "(host)", len(cand)))
    assert len(cand) >= 10
    H.check(g, pods, done, D, WLOG2, P, cms, cand, want=None if want_h is None else (cms, want_h))
    info = g.hh_info()
    assert {k: info[k] for k in INFO} == INFO, info


# ---- the state is cleared: the waiting lists go with it ---------------------------------------
def reset(be, flags: int):
    pods, p1, p2, _ = parts()
    cms, cand = H.restate([p2], D, WLOG2, T)
    assert cand != H.restate([p1], D, WLOG2, T)[1] and cand != H.restate([p1, p2], D, WLOG2, T)[1]
    g = engine(be, pods, flags)
    try:
        keep = [be.submit(g, p1)]
        g.reset()
        assert g.hh_info() == dict(INFO, candidates=0, dropped=0)
        keep.append(be.submit(g, p2))
        finish(g, pods, [p2], cms, cand)
        del keep
    finally:
        g.close()


def reconcile(be, flags: int, same: bool):
    """The same options as a set (the labels in another order) leave everything alone; other
    options clear the state -- rows, registers, candidates -- and keep min_count."""
    pods, p1, p2, _ = parts()
    done = [p1, p2] if same else [p2]
    cms, cand = H.restate(done, D, WLOG2, T)
    g = engine(be, pods, flags)
    try:
        keep = [be.submit(g, p1)]
        g.reconcile(SAME_SPEC if same else OTHER_SPEC)
        if not same:  # (hh_info reads the table alone: it folds nothing)
            assert g.hh_info() == dict(INFO, candidates=0, dropped=0)
        keep.append(be.submit(g, p2))
        finish(g, pods, done, cms, cand)
        del keep
    finally:
        g.close()


# ---- the slot table grows: the registers are laid out again, kept ---------------------------------
def load_endpoints(be, flags: int):
    """100 more pods: key_cap grows from 128 to 256 slots and the HLL rows move (layout_dense
    with keep), which has to fold part 1 -- under the slot map it was scattered with --
    first.  A tenth of part 2 comes from the new pods."""
    pods, p1, base2, _ = parts()
    new = [W.Endpoint("ns-more", "more-%d" % i, [W.ip_le(10, 9, 0, i)], None) for i in range(100)]
    p2 = copy_of(base2)
    p2.src_ip[::10] = np.array([e.ips[0] for e in new], np.uint32)[np.arange(len(p2.src_ip[::10])) % 100]
    both = slot_map([e.ips for e in pods.endpoints] + [e.ips for e in new])
    cms, cand = H.restate([p1, p2], D, WLOG2, T)
    want_h = registers(200, (pods, p1), (both, p2))
    assert want_h[100:].any() and (K.src_slots(pods, p2.src_ip) != K.src_slots(both, p2.src_ip)).any()
    g = engine(be, pods, flags, max_slots=2048, max_ips=4096)
    try:
        keep = [be.submit(g, p1)]
        g.load_endpoints(new, version=2)
        keep.append(be.submit(g, p2))
        finish(g, both, [p1, p2], cms, cand, want_h)
        assert g.hll_array().shape[0] == 256
        del keep
    finally:
        g.close()


# ---- slots retire: their registers are zeroed after part 1 is in them ---------------------------
def retire(be, flags: int):
    """Every third pod (1, 4, 7, ...) is deleted and its slot retired: its HLL row is zero and
    its estimates are 0.0, the other rows hold part 1, the count-min rows and the candidates
    are untouched (flows are keyed by address).  A new pod then takes the lowest freed slot, 1;
    part 2 carries its traffic and its row holds nothing else."""
    pods, p1, base2, _ = parts()
    gone = list(range(1, 100, 3))
    new_ip = W.ip_le(10, 250, 0, 1)
    p2 = copy_of(base2)
    p2.src_ip[::10] = new_ip
    after = [[] if s in gone else e.ips for s, e in enumerate(pods.endpoints)]
    after[gone[0]] = [new_ip]
    after = slot_map(after)
    cms1, cand1 = H.restate([p1], D, WLOG2, T)
    h1 = registers(100, (pods, p1))
    assert h1[gone].any(axis=1).all(), "every pod that leaves has registers to lose"
    h1[gone] = 0
    g = engine(be, pods, flags)
    try:
        keep = [be.submit(g, p1)]
        for s in gone:
            g.cache_delete_endpoint(pods.endpoints[s].namespace, pods.endpoints[s].name)
        g.cache_commit(2)
        assert g.retire_slots() == len(gone)
        est = g.hll_estimates()
        g.sketch_refresh()
        assert (est[gone] == 0.0).all() and all(g.hll_estimate(s) == 0.0 for s in gone)
        live = np.setdiff1d(np.arange(100), gone)
        assert (est[live] > 0.0).all()
        H.check(g, pods, [p1], D, WLOG2, P, cms1, cand1, want=(cms1, h1))
        g.cache_update_endpoint(W.Endpoint("ns-new", "pod-new", [new_ip], None))
        g.cache_commit(3)
        keep.append(be.submit(g, p2))
        cms, cand = H.restate([p1, p2], D, WLOG2, T)
        want_h = h1.copy()
        S.hll_update(want_h, K.src_slots(after, p2.src_ip), p2.dst_ip, P)
        only = registers(100, (after, p2))
        assert np.array_equal(want_h[gone[0]], only[gone[0]]) and only[gone[0]].any()
        finish(g, after, [p1, p2], cms, cand, want_h)
        assert not g.hll_array()[gone[1:]].any()
        del keep
    finally:
        g.close()


# ---- a second engine is merged in: both unsynced and unread ---------------------------------------
def merge(be, flags: int, peer: bool):
    """Rows the sum, registers the row-wise maximum, candidates the union (estimates from the
    summed rows); the source reads back zero.  peer: GPUAGG_MERGE=peer -- contexts on one
    device take the peer-copy path either way, the variable must not change that."""
    pods, p1, p2, p3 = parts()
    (cms1, cand1), (cms3, cand3) = H.restate([p1], D, WLOG2, T), H.restate([p3], D, WLOG2, T)
    assert cand1 - cand3 and cand3 - cand1
    cms, cand = cms1 + cms3, cand1 | cand3
    key = H.keys_of(p2)
    S.cms_update(cms, key[:, 0], key[:, 1], key[:, 2], key[:, 3])
    uniq = np.unique(key, axis=0)
    cand |= H.as_set(uniq[H.estimate(cms, uniq) >= T])
    old = os.environ.get("GPUAGG_MERGE")
    if peer:
        os.environ["GPUAGG_MERGE"] = "peer"
    gs = [engine(be, pods, flags), engine(be, pods, flags)]
    try:
        keep = [be.submit(gs[0], p1), be.submit(gs[1], p3)]
        gs[0].merge_from([gs[1]])
        assert not gs[1].cms_array().any() and not gs[1].hll_array().any()
        assert gs[1].hh_info() == dict(INFO, candidates=0, dropped=0) and len(gs[1].hh_candidates()) == 0
        keep.append(be.submit(gs[0], p2))
        finish(gs[0], pods, [p1, p3, p2], cms, cand)
        del keep
    finally:
        for g in gs:
            g.close()
        if peer:
            if old is None:
                del os.environ["GPUAGG_MERGE"]
            else:
                os.environ["GPUAGG_MERGE"] = old


# ---- reads: as if nothing had happened ------------------------------------------------------------
READS = ["snapshot", "snapshot_delta", "hll_estimates", "heavy_hitters", "add_present"]


def read(be, flags: int, which: str):
    """A read between the parts is the first thing to touch the waiting lists; what it returns
    is part 1's, and the end state is parts 1 + 2."""
    pods, p1, p2, _ = parts()
    cms1, cand1 = H.restate([p1], D, WLOG2, T)
    cms, cand = H.restate([p1, p2], D, WLOG2, T)
    g = engine(be, pods, flags)
    try:
        keep = [be.submit(g, p1)]
        if which == "snapshot":
            assert sum(g.snapshot().values()) > 0
        elif which == "snapshot_delta":
            delta, rebased = g.snapshot_delta()
            assert rebased and sum(delta.values()) > 0
        elif which == "hll_estimates":
            est, h1 = g.hll_estimates(), registers(100, (pods, p1))
            for s in range(100):
                want = S.hll_estimate(h1[s])
                assert abs(est[s] - want) <= K.HLL_EST_TOL * want, (s, est[s], want)
        elif which == "heavy_hitters":
            assert H.rows(g.heavy_hitters(4)) == H.topk(cms1, cand1, 4)
        else:
            g.hh_add_candidates(np.array(sorted(cand1), np.uint32))
            assert H.candidates(g) == cand1
        keep.append(be.submit(g, p2))
        finish(g, pods, [p1, p2], cms, cand)
        del keep
    finally:
        g.close()
