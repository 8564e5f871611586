"""What the heavy-hitter candidate pass costs a submit, and what the on-device distinct-peer
readout saves, on one MI355X (a diagnostic, not the bench).

C3's sketch configuration (LOCAL_FWD_DROP metrics, count-min d = 4, w = 2^20, HLL p = 14,
10k pods) and C3's records (10^7 flows, sources in the pods), 2^24 of them resident in HBM.
A leg is: gpuagg_reset, gpuagg_set_heavy_hitters (off: never called), --warmup synced
submits, then --runs timed ones -- wall clock around gpuagg_submit_device + gpuagg_sync, the
stream idle before it.  The legs "off" and "on" alternate --rounds times in this one process.

min_count is the count-min's own error bound for the leg, eps * N with eps = e / w and N the
records the leg submits ((warmup + runs) * records): a key reaches it only if it is heavier
than what collisions alone can add, which is the threshold a user of this sketch would pick.

Then the distinct-peer readout at the same shape: gpuagg_hll_estimate_all against
gpuagg_sketch_refresh + one gpuagg_hll_estimate per pod (through ctypes, as a Python caller
pays it).

One JSON line per leg and readout, then a summary line: the medians, on / off, and the off
legs' own run-to-run spread (the bar for a comparison with another build's off leg).  A
library without the new entry points (the parent commit: put its checkout first on
PYTHONPATH) runs the off legs and the refresh path only.
"""

import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)  # (behind PYTHONPATH: another checkout's retina_amd may be measured)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from retina_amd import GpuAgg  # noqa: E402
from retina_amd import workloads as W  # noqa: E402

CMS_DEPTH, CMS_WIDTH_LOG2, HLL_P, PODS = 4, 20, 14, 10_000


def gen_device_records(n, pods, seed, device, gen_kw, chunk=8_000_000):
    """bench.py's generator: host chunks of seed * 1000 + k, resident in HBM."""
    cols = [torch.empty(n, dtype=torch.int32, device=device) for _ in range(6)]
    for k, start in enumerate(range(0, n, chunk)):
        m = min(chunk, n - start)
        r = W.gen_records(m, pods, seed * 1000 + k, **gen_kw)
        for t, a in zip(cols, (r.src_ip, r.dst_ip, r.bytes, r.meta, r.ports, r.dns_id)):
            t[start:start + m].copy_(torch.from_numpy(a.view(np.int32)))
    return cols


def spread(ts):
    q = statistics.quantiles(ts, n=4) if len(ts) >= 4 else [min(ts), statistics.median(ts), max(ts)]
    return dict(median_ms=round(1e3 * statistics.median(ts), 4), min_ms=round(1e3 * min(ts), 4),
                max_ms=round(1e3 * max(ts), 4), iqr_ms=round(1e3 * (q[2] - q[0]), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--capacity-log2", type=int, default=0)
    a = ap.parse_args()
    have = hasattr(GpuAgg, "set_heavy_hitters")
    dev = torch.device("cuda", 0)
    pods = W.make_pods(PODS, seed=3)
    cols = gen_device_records(a.records, pods, 3, dev, dict(W.CONFIGS["c3"]["gen"]))
    g = GpuAgg(device=0, max_slots=len(pods.endpoints) + 64, max_ips=len(pods.ips), cms_depth=CMS_DEPTH,
               cms_width_log2=CMS_WIDTH_LOG2, hll_precision=HLL_P)
    g.reconcile(W.LOCAL_FWD_DROP)
    g.load_endpoints(pods.endpoints)
    dcols = GpuAgg.device_columns(*cols)
    n_leg = (a.warmup + a.runs) * a.records
    min_count = math.ceil(math.e / (1 << CMS_WIDTH_LOG2) * n_leg)
    build = g.lib.gpuagg_build_id().decode()

    def submit():
        torch.cuda.synchronize()
        t = time.perf_counter()
        g.submit_device(dcols, a.records)
        g.sync()
        return time.perf_counter() - t

    med = {"off": [], "on": []}
    iqr_off = []
    for rnd in range(a.rounds):
        for leg in ("off", "on") if have else ("off",):
            g.reset()
            if have:
                g.set_heavy_hitters(min_count if leg == "on" else 0, a.capacity_log2)
            for _ in range(a.warmup):
                submit()
            ts = [submit() for _ in range(a.runs)]
            row = dict(row="submit", leg=leg, round=rnd, records=a.records, build=build, **spread(ts))
            if leg == "on":
                row.update(g.hh_info())
            else:
                iqr_off.append(row["iqr_ms"])
            med[leg].append(row["median_ms"])
            print(json.dumps(row), flush=True)

    # the distinct-peer readout: the state of the last leg (every pod has sent)
    slots = len(pods.endpoints)
    refresh, allcall = [], []
    for _ in range(5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        g.sketch_refresh()
        one = [g.hll_estimate(s) for s in range(slots)]
        refresh.append(time.perf_counter() - t)
        if have:
            t = time.perf_counter()
            est = g.hll_estimates()
            allcall.append(time.perf_counter() - t)
            assert np.allclose(est[:slots], one, rtol=1e-9, atol=0)
    print(json.dumps(dict(row="hll", path="refresh+estimate", pods=slots, p=HLL_P, build=build, **spread(refresh))),
          flush=True)
    if have:
        print(json.dumps(dict(row="hll", path="estimate_all", pods=slots, p=HLL_P, build=build, **spread(allcall))),
              flush=True)
    out = dict(row="summary", build=build, records=a.records, off_median_ms=round(statistics.median(med["off"]), 4),
               off_medians_ms=med["off"], off_iqr_ms=max(iqr_off),
               off_round_to_round_ms=round(max(med["off"]) - min(med["off"]), 4))
    if have:
        out.update(on_median_ms=round(statistics.median(med["on"]), 4), on_medians_ms=med["on"],
                   on_over_off=round(statistics.median(med["on"]) / statistics.median(med["off"]), 4),
                   min_count=min_count,
                   hll_all_over_refresh=round(statistics.median(allcall) / statistics.median(refresh), 6))
    print(json.dumps(out), flush=True)
    g.close()


if __name__ == "__main__":
    main()
