"""Both HBM images of the IP -> pod map agree with the oracle: the radix table (pod IPs
in few /16 prefixes, the default for cluster CIDRs) and the bucketized cuckoo table
(IPs spread over more than 64 prefixes, or GPUAGG_FLAG_NO_RADIX_IP_TABLE).  Then every
device form of the lookup -- three HBM forms, three LDS images, 8-wide and one-IP probes --
under every kernel that reaches it, with records whose addresses almost match a pod, the
kernel asserted by name; across table swaps that change the form; in enrich_kernel and in
the sketch pass."""

import numpy as np
import pytest

from retina_amd import workloads as W

from .helpers import diff_series, engine_series, oracle_series

pytestmark = pytest.mark.gpu


def _scattered_pods(n, seed):
    """Pods whose IPs span thousands of /16 prefixes (radix table not applicable)."""
    pods = W.make_pods(n, seed=seed)
    rng = np.random.default_rng(seed)
    remap = {}
    for ip in pods.ips.tolist():
        remap[ip] = int(rng.integers(1, 2**32 - 1))
    eps = [W.Endpoint(e.namespace, e.name, [remap[x] for x in e.ips], e.owner_refs) for e in pods.endpoints]
    ips = np.array([remap[x] for x in pods.ips.tolist()], np.uint32)
    return W.Pods(eps, ips, pods.ip_owner)


@pytest.mark.parametrize("layout", ["radix", "bucket-flag", "bucket-scattered"])
@pytest.mark.parametrize("remote,spec", [(False, W.LOCAL_FWD_DROP + W.C5_SPEC), (True, W.C1_REMOTE)],
                         ids=["local", "remote"])
def test_ip_table_layouts(gpu_device, layout, remote, spec):
    pods = _scattered_pods(3000, 5) if layout == "bucket-scattered" else W.make_pods(3000, seed=5)
    recs = W.gen_records(80_000, pods, seed=6, drop_frac=0.1, retrans_frac=0.05, dns_frac=0.1,
                         udp_frac=0.1, n_queries=300)
    kw = {"flags": 4} if layout == "bucket-flag" else {}
    got = engine_series(recs, pods, spec, remote, gpu_device, host_fed=False, **kw)
    want = oracle_series(recs, pods, spec, remote)
    assert got == want, diff_series(got, want)
    assert len(want) > 100


# ---- every form of the lookup under every kernel, near-miss addresses -----------------------
# (tests/iptable_cases.py: the pod sets, the records and the table with the kernel names)
from . import iptable_cases as IC  # noqa: E402


@pytest.mark.parametrize("case", IC.CASES, ids=[c.id for c in IC.CASES])
def test_lookup_forms_vs_oracle(gpu_device, case):
    """One batch of near-miss records through the form and kernel the case names: series
    equal to the oracle's, nothing lost, and the kernel that ran is the one expected."""
    got, kernel, stats = IC.run_case(case, gpu_device)
    want = IC.want_series(case.pods, case.n, case.spec, case.remote)
    print("%s: %s" % (case.id, kernel))
    assert got == want, diff_series(got, want)
    assert kernel == case.kernel
    assert stats["sparse_dropped"] == 0 and len(want) > 100


@pytest.mark.parametrize("n", [4000, 4001])  # vector path + a ragged tail
@pytest.mark.parametrize("npfx", [1, 9, 64, 65])  # enrich_kernel: the `pre` table up to 64 prefixes, then buckets
def test_enrich_near_miss(gpu_device, npfx, n):
    """enrich_kernel's slots of near-miss records, slot by slot against the oracle's
    Enricher; a service and a node own pod-range IPs (GetObjByIP finds them: no endpoint)."""
    import torch
    from oracle import oracle as O
    from .helpers import oracle_cache
    from .test_gpu_enrich import _run, _want
    pods, base, _ = IC.inputs((npfx, "run"), n)
    svc_ip, node_ip = int(pods.ips[5]), int(pods.ips[7])
    src, dst = base.src_ip.copy(), base.dst_ip.copy()
    src[100:104], dst[100:104] = svc_ip, node_ip  # (one whole vector of each, and the last record)
    src[-1], dst[-1] = node_ip, svc_ip
    recs = W.Records(src, dst, base.bytes, base.meta, base.ports, base.dns_id, base.dns)
    g = IC.make_case_engine(pods, [], False, 0, gpu_device, recs)
    try:
        g.cache_update_service("ns-svc", "svc-a", svc_ip)
        g.cache_update_node("node-a", node_ip)
        g.cache_commit(1)
        slot_of = {}
        for ep in pods.endpoints:
            own = ep.owner_refs[0] if ep.owner_refs else (None, None)
            slot_of[(ep.namespace, ep.name)] = g.slot_intern(ep.namespace, ep.name, own[0], own[1])
        got = _run(g, recs, torch.device("cuda", gpu_device))
    finally:
        g.close()
    cache = oracle_cache(pods)
    cache.update_retina_svc(O.RetinaSvc("svc-a", "ns-svc", O.int2ip(svc_ip)))
    cache.update_retina_node(O.RetinaNode("node-a", O.int2ip(node_ip)))
    ws, wd = _want(cache, recs, slot_of)
    for w, col in ((ws, recs.src_ip), (wd, recs.dst_ip)):
        assert (w == -1).mean() > 0.25 and (w >= 0).mean() > 0.25
        assert (w[np.isin(col, [svc_ip, node_ip])] == -1).all() and np.isin(col, [svc_ip, node_ip]).any()
    np.testing.assert_array_equal(got[0], ws)
    np.testing.assert_array_equal(got[1], wd)


SWAP_CASES = [
    ("local-lds", "lds", "fwd-drop", False,
     ["dense_lds_kernel<2, true, 169u, 2>", "dense_lds_kernel<2, true, 169u, 0>", "dense_lds_kernel<2, true, 169u, 2>"]),
    ("remote-lds", "lds", "c1-remote", True,
     ["wide_kernel<2, true, true, 2>", "wide_kernel<2, true, true, 0>", "wide_kernel<2, true, true, 2>"]),
    ("local-hbm", "hbm", "fwd-drop", False, ["dense_local_kernel<2, true, false, 0u>"] * 3),
    ("generic-hbm", "hbm", "c1-local", False, ["wide_kernel<2, false, true, -1>"] * 3),
]


@pytest.mark.parametrize("cid,kind,spec,remote,kernels", SWAP_CASES, ids=[c[0] for c in SWAP_CASES])
def test_swap_across_forms(gpu_device, cid, kind, spec, remote, kernels):
    """One engine, three batches, the table swapped between them across a change of form
    (4 -> 5 -> 1 prefixes: dense radix -> cuckoo -> dense radix image; 8 -> 9 -> 65 without
    LDS images: compares -> `pre` table -> buckets).  Each batch carries addresses of the
    generation before, which now belong to other pods or to none."""
    got, names, stats = IC.run_swap(kind, spec, remote, gpu_device)
    want = IC.want_swap(kind, spec, remote)
    print("%s: %s" % (cid, names))
    assert got == want, diff_series(got, want)
    assert names == kernels
    assert stats["sparse_dropped"] == 0 and len(want) > 100


@pytest.mark.parametrize("cid,key,flags,unaligned,kernel", IC.HLL_CASES, ids=[c[0] for c in IC.HLL_CASES])
def test_hll_sources_near_miss(gpu_device, cid, key, flags, unaligned, kernel):
    """The sketch pass resolves the source pod through the all-pods image (the apiserver
    pseudo pod included) or the HBM table: HLL registers at p = 8 bit for bit against
    oracle.sketch.hll_update with the slots from a dict, near-miss sources updating none."""
    from . import sketch_cases as SC
    pods, recs = IC.hll_inputs(key, unaligned)
    ip_slot = {int(ep.ips[0]): s for s, ep in enumerate(pods.endpoints)}
    slot = np.array([ip_slot.get(int(x), -1) for x in recs.src_ip], np.int64)
    assert np.array_equal(slot, SC.src_slots(pods, recs.src_ip)) and (slot == 0).any()  # (0: the apiserver pod)
    SC.run(SC.Backend(gpu_device), pods, [recs], 0, 0, 8, flags, kernel, unaligned=unaligned,
           sparse_capacity_log2=16)
