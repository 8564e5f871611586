"""Inputs and checks shared by the group-by table growth tests (GPU and CPU backend):
the seeded workloads, the C-port reference of each (computed once per process) and the
table export as canonical entries."""

from __future__ import annotations

import functools
import zlib

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


# the specs of test_gpu_parity.CASES the growth tests run (that module's record recipe):
# wide keys with ports and DNS ids (the all6 ones), dense groups beside wide keys
# (local-all6), the compact layout (c5-local), edge rows (odd-rows-remote)
PARITY = ("local-c1-ip-ns-pod-wl", "local-all6", "remote-plain", "remote-all6-both", "c5-local",
          "odd-rows-remote")


@functools.lru_cache(maxsize=None)
def _parity_pods():
    return W.make_pods(400, seed=11)


def _parity(cid):
    from .test_gpu_parity import CASES
    _, spec, remote, gen = next(c for c in CASES if c[0] == cid)
    pods = _parity_pods()
    return pods, W.gen_records(30_000, pods, seed=zlib.crc32(cid.encode()) & 0xFFFF, **gen), spec, remote


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
    pods, recs, spec, remote = _INPUTS[name]() if name in _INPUTS else _parity(name)
    r = RefCPU(spec, pods.endpoints, remote, recs.dns)
    r.process(recs)
    want = r.series()
    r.close()
    return pods, recs, spec, remote, want


def ref_series(pods, recs, spec, remote):
    """The C port's series of one batch."""
    r = RefCPU(spec, pods.endpoints, remote, recs.dns)
    r.process(recs)
    want = r.series()
    r.close()
    return want


def take(recs: W.Records, idx) -> W.Records:
    """The rows `idx` (an index array or a slice) of a batch, with its DNS payloads."""
    return W.Records(recs.src_ip[idx], recs.dst_ip[idx], recs.bytes[idx], recs.meta[idx], recs.ports[idx],
                     recs.dns_id[idx], recs.dns)


def slices(recs: W.Records, chunks):
    """`chunks` equal slices, or -- a sequence -- slices of these lengths."""
    if isinstance(chunks, int):
        bounds = np.linspace(0, len(recs), chunks + 1).astype(int)
    else:
        bounds = np.concatenate([[0], np.cumsum(chunks)]).astype(int)
        assert bounds[-1] == len(recs)
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


def dns_updates(want) -> int:
    """The DNS request / response updates behind a reference series dict."""
    return sum(v for (metric, _), v in want.items() if "_dns_re" in metric)


# ---- wide list entries: the packed count and byte fields --------------------------------
# (gpuagg_internal.h) a list entry's last word is home:12 | count:12 | bytes:40, so an update
# fits it while count < 2^(kWideHomeShift - kWideCountShift) and bytes < 2^kWideCountShift
WIDE_COUNT_LIMIT = 1 << (52 - 40)
WIDE_BYTES_LIMIT = 1 << 40
WIDE_BYTES = (1, (1 << 20) - 1, 1 << 24, (1 << 31) + 5, (1 << 32) - 1)


@functools.lru_cache(maxsize=None)
def wide_field_rows():
    """(pods, rows): three remote-context keys of C1_REMOTE over 10,000 pods -- row 0 a
    forwarded and row 1 a dropped pod -> pod record picked from gen_records, row 2 the
    forwarded one towards an address that is no pod's."""
    pods = W.make_pods(10_000, seed=5)
    base = W.gen_records(400, pods, seed=5, pod_frac=1.0, drop_frac=0.5)
    verdict = (base.meta >> 8) & 0xFF
    ok = base.src_ip != base.dst_ip
    f = int(np.flatnonzero((verdict == W.V_FWD) & ok)[0])
    d = int(np.flatnonzero((verdict == W.V_DROP) & ok)[0])
    rows = take(base, np.array([f, d, f]))
    rows.dst_ip[2] = W.ip_le(100, 64, 0, 1)
    assert rows.dst_ip[2] not in set(pods.ips.tolist())
    return pods, rows


def wide_field_batch(key_ids, nbytes) -> W.Records:
    """The batch whose record j is wide_field_rows() row key_ids[j] with nbytes[j] bytes."""
    _, rows = wide_field_rows()
    out = take(rows, np.asarray(key_ids))
    out.bytes = np.asarray(nbytes, np.uint32)
    return out


def scale_series(series, reps: int):
    return {k: v * reps for k, v in series.items()}
