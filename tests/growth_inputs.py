"""Inputs and checks shared by the group-by table growth tests (GPU and CPU backend):
the seeded workloads, the C-port reference of each (computed once per process) and the
table export as canonical entries."""

from __future__ import annotations

import functools

import numpy as np

from oracle.ref_cpu import RefCPU, values_only
from retina_amd import workloads as W

# name -> (pods, records, spec, remote context)
_INPUTS = {
    # the input of test_full_table_reports_loss: 17,421 keys
    "small-wide": lambda: _wide(W.make_pods(100, seed=95), lambda p: W.gen_records(20_000, p, seed=96)),
    # 329,728 distinct wide keys, every flow its own key
    "many-wide": lambda: _wide(W.make_pods(10_000, seed=12),
                               lambda p: W.gen_records(400_000, p, seed=131, flows=400_000, flow_zipf=None,
                                                       n_dst=1_000_000)),
    # compact (64-bit DNS) keys
    "compact": lambda: _compact(),
}


def _wide(pods, gen):
    return pods, gen(pods), W.C1_REMOTE, True


def _compact():
    pods = W.make_pods(2_000, seed=3)
    recs = W.gen_records(300_000, pods, seed=3, drop_frac=0.0, retrans_frac=0.05, dns_frac=0.5, n_queries=50_000)
    return pods, recs, W.C5_SPEC, False


@functools.lru_cache(maxsize=None)
def workload(name: str):
    """(pods, records, spec, remote, reference series) of one input; the reference is the C
    port's (RefCPU), left unchanged for every test that compares against it."""
    pods, recs, spec, remote = _INPUTS[name]()
    r = RefCPU(spec, pods.endpoints, remote, recs.dns)
    r.process(recs)
    want = r.series()
    r.close()
    return pods, recs, spec, remote, want


def slices(recs: W.Records, chunks: int):
    bounds = np.linspace(0, len(recs), chunks + 1).astype(int)
    for a, b in zip(bounds[:-1], bounds[1:]):
        yield W.Records(recs.src_ip[a:b], recs.dst_ip[a:b], recs.bytes[a:b], recs.meta[a:b], recs.ports[a:b],
                        recs.dns_id[a:b])


def canonical(entries: np.ndarray):
    """(n, 5) exported entries -> {(k0, k1, k2): (count, bytes)}, duplicate slots summed."""
    out = {}
    for k0, k1, k2, c, b in entries.tolist():
        pc, pb = out.get((k0, k1, k2), (0, 0))
        out[(k0, k1, k2)] = (pc + c, pb + b)
    return out


def snapshot_values(g):
    return values_only(g.snapshot())
