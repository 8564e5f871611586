"""Scrape cost of the full snapshot against delta snapshots on one MI355X (a diagnostic, not
the bench).

Builds the c4-remote workload at the size tests/test_gpu_scale.py runs it (100M Zipf(1.2)
flow records, 10k pods, C1_REMOTE, a 2^24-slot table), submits it and times, each as the
median of --runs runs (wall clock around the C call, the stream idle before it):

  full          gpuagg_snapshot + gpuagg_result_count
  delta-rebased gpuagg_snapshot_delta on a fresh baseline (after gpuagg_reset and the same
                submit): every entry is "changed"
  delta-10%     a delta after re-submitting a prefix of the records that touches about a
  delta-1%      tenth / a hundredth of the keys (the share the scan reports is printed)
  delta-idle    a delta with nothing submitted in between: the device scans, two stream
                synchronisations and no host work -- an upper bound of the scan kernels

One JSON line per row.  --full-only stops after the first (a library without the delta
entry points, for the parent's number).
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)  # (behind PYTHONPATH: another checkout's retina_amd may be measured)

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from retina_amd import GpuAgg  # noqa: E402
from retina_amd import workloads as W  # noqa: E402


def gen_device_records(n, pods, seed, device, gen_kw, chunk=8_000_000):
    """bench.py's generator: host chunks of seed * 1000 + k, resident in HBM."""
    cols = [torch.empty(n, dtype=torch.int32, device=device) for _ in range(6)]
    for k, start in enumerate(range(0, n, chunk)):
        m = min(chunk, n - start)
        r = W.gen_records(m, pods, seed * 1000 + k, **gen_kw)
        for t, a in zip(cols, (r.src_ip, r.dst_ip, r.bytes, r.meta, r.ports, r.dns_id)):
            t[start:start + m].copy_(torch.from_numpy(a.view(np.int32)))
    return cols


def prefix_for(first_chunk, keys):
    """Rows of the first chunk whose (src, dst) pairs number about `keys`."""
    pair = first_chunk.src_ip.astype(np.uint64) << np.uint64(32) | first_chunk.dst_ip.astype(np.uint64)
    _, first = np.unique(pair, return_index=True)
    first.sort()
    return len(pair) if keys >= len(first) else int(first[keys])


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--full-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    pods = W.make_pods(10_000, seed=4)
    gen = dict(W.CONFIGS["c4"]["gen"])
    cols = gen_device_records(a.records, pods, 4, dev, gen)
    g = GpuAgg(device=0, remote_context=True, max_slots=len(pods.endpoints) + 64, max_ips=len(pods.ips),
               sparse_capacity_log2=24)
    g.reconcile(W.C1_REMOTE)
    g.load_endpoints(pods.endpoints)

    def submit(n):
        g.submit_device(GpuAgg.device_columns(*cols), n)
        g.sync()

    def row(name, times, **kw):
        print(json.dumps(dict(row=name, median_s=round(statistics.median(times), 4),
                              runs=[round(t, 4) for t in times], **kw)), flush=True)

    def full():
        r = C.c_void_p()
        g._check(g.lib.gpuagg_snapshot(g.h, C.byref(r)))
        return r, int(g.lib.gpuagg_result_count(r))

    submit(a.records)
    times = []
    for _ in range(a.runs + 1):  # (the first one faults the scrape buffers in: dropped)
        t, (r, series) = timed(full)
        g.lib.gpuagg_result_free(r)
        times.append(t)
    row("full", times[1:], series=series, first_s=round(times[0], 4))
    if a.full_only:
        g.close()
        return

    times, info = [], {}
    for _ in range(a.runs + 1):
        g.reset()
        submit(a.records)
        t, (n, rebased) = timed(g.snapshot_delta_count)
        assert rebased and n == series, (n, series, rebased)
        times.append(t)
        info = g.delta_info()
    entries = info["changed_entries"]
    row("delta-rebased", times[1:], series=n, first_s=round(times[0], 4), **info)

    first_chunk = W.gen_records(min(8_000_000, a.records), pods, 4000, **gen)
    for name, share in (("delta-10%", 0.10), ("delta-1%", 0.01)):
        m = prefix_for(first_chunk, int(entries * share))
        times, shares, ns = [], [], []
        for _ in range(a.runs):
            submit(m)
            t, (n, rebased) = timed(g.snapshot_delta_count)
            assert not rebased
            times.append(t)
            ns.append(n)
            shares.append(g.delta_info()["changed_entries"] / entries)
        row(name, times, records=m, series=ns[-1], changed_share=round(statistics.median(shares), 4))

    times = []
    for _ in range(a.runs):
        t, (n, rebased) = timed(g.snapshot_delta_count)
        assert n == 0 and not rebased
        times.append(t)
    row("delta-idle", times, **g.delta_info())
    g.close()


if __name__ == "__main__":
    main()
