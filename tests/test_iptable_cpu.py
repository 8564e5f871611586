"""The IP -> pod lookup cases of tests/iptable_cases.py without a GPU: every row of the
table through GPUAGG_FLAG_CPU_BACKEND against the oracle (the inputs and the oracle agree
before a device sees them, and the host radix mirror of gpuagg_cpu.cpp is crossed at 8/9
and 64/65 prefixes), the near-miss records' own statistics, and the host mirrors of the
three LDS image probes (ipl_build.h) on the cases' pod sets with every near-miss class as
an absent probe."""

import numpy as np
import pytest

from retina_amd import workloads as W

from . import iptable_cases as IC
from .helpers import diff_series
from .test_ipl_build import harness, run_sets  # noqa: F401  (harness: the g++-built fixture)


@pytest.fixture(scope="module", autouse=True)
def lib():
    from retina_amd import _abi, build
    build.build()
    return _abi.load()


@pytest.mark.parametrize("case", IC.CASES, ids=[c.id for c in IC.CASES])
def test_cases_vs_oracle_cpu_backend(case):
    got, kernel, stats = IC.run_case(case, device=None)
    want = IC.want_series(case.pods, case.n, case.spec, case.remote)
    assert got == want, diff_series(got, want)
    assert kernel == "cpu"
    assert stats["sparse_dropped"] == 0 and len(want) > 100


@pytest.mark.parametrize("kind,spec,remote", [("lds", "fwd-drop", False), ("lds", "c1-remote", True),
                                              ("hbm", "fwd-drop", False), ("hbm", "c1-local", False)])
def test_swap_sequences_cpu_backend(kind, spec, remote):
    """The three generations of the swap tests, the tables swapped between the batches:
    engine and oracle agree on the sequence before a device runs it."""
    got, names, stats = IC.run_swap(kind, spec, remote, None)
    want = IC.want_swap(kind, spec, remote)
    assert got == want, diff_series(got, want)
    assert names == ["cpu"] * 3
    assert stats["sparse_dropped"] == 0 and len(want) > 100
    prefixes = [len(np.unique(p.ips & np.uint32(0xFFFF))) for p, _ in IC.swap_batches(kind)]
    assert prefixes == {"lds": [4, 5, 1], "hbm": [8, 9, 65]}[kind]
    for (prev, _), (pods, recs) in zip(IC.swap_batches(kind), IC.swap_batches(kind)[1:]):
        stale = np.isin(recs.src_ip, prev.ips) & ~np.isin(recs.src_ip, pods.ips)
        moved = np.isin(recs.src_ip, prev.ips) & np.isin(recs.src_ip, pods.ips)
        assert stale.sum() + moved.sum() > 100  # addresses a stale table would answer differently


PODS_KEYS = sorted({(c.pods, c.n) for c in IC.CASES}, key=repr)


@pytest.mark.parametrize("key,n", PODS_KEYS, ids=["%s-%d" % (k if isinstance(k, str) else "-".join(map(str, k)), n)
                                                  for k, n in PODS_KEYS])
def test_near_miss_self_checks(key, n):
    """Every mutation class at least 20 times in each column, a quarter to three quarters
    of the sources no pod -- and the mutated columns still hold pods' own addresses, pods
    reached through a mutation (another pod of the same /24) and all eight classes' values."""
    pods, recs, st = IC.inputs(key, n)
    IC.check_mutation_stats(st)
    assert len(recs) == n
    for col in (recs.src_ip, recs.dst_ip):
        assert np.isin(col, pods.ips).mean() > 0.25
        assert (col == 0xFFFFFFFF).sum() >= IC.MIN_PER_CLASS and (col == 0).sum() >= IC.MIN_PER_CLASS
    if key != "scattered":  # same /16 as a pod, but no pod: what the radix forms must refuse
        pfx = np.unique(pods.ips & np.uint32(0xFFFF))
        near = np.isin(recs.src_ip & np.uint32(0xFFFF), pfx) & ~np.isin(recs.src_ip, pods.ips)
        assert near.sum() >= 4 * IC.MIN_PER_CLASS


def test_table_reaches_every_form():
    """The kernel names the table asserts: every dense_lds_kernel kIp and every wide_kernel
    kip, and dense_local_kernel and aggregate_kernel over the three HBM forms -- each with
    vector and with scalar loads where the kernel has both."""
    names = {c.kernel for c in IC.CASES}
    for kip in (0, 1, 2):
        for vec in ("true", "false"):
            assert "dense_lds_kernel<2, %s, 169u, %d>" % (vec, kip) in names
    for kip in (-1, 0, 1, 2):
        assert "wide_kernel<2, true, true, %d>" % kip in names
    hbm = {"compare": (1, 4, 8), "pre": (9, 64), "bucket": (65, "scattered")}
    for kernel in ("dense_local_kernel<2, %s, false, 0u>", "aggregate_kernel<%s, false>"):
        for form, sets in hbm.items():
            for vec in ("true", "false"):
                rows = [c for c in IC.CASES if c.kernel == kernel % vec and not c.remote
                        and not c.flags & IC.NO_RADIX and (c.pods if isinstance(c.pods, str) else c.pods[0]) in sets]
                assert rows, (kernel % vec, form)
    # forced and natural selection of the LDS forms
    by_id = {c.id: c for c in IC.CASES}
    assert by_id["t1-cuckoo-5-vec-tail"].flags == 0 and by_id["t1-row-too-wide-scalar"].flags == 0
    tails = {c.kernel.split("<")[0] for c in IC.CASES if c.n % 4 and c.align == "vec"}
    assert tails == {"dense_lds_kernel", "dense_local_kernel", "aggregate_kernel", "wide_kernel"}
    assert max(len(IC.pods_of(c.pods).ips) for c in IC.CASES) <= 2600 and max(c.n for c in IC.CASES) <= 4003


# ---- host mirrors of the LDS image probes ---------------------------------------------------

def _absent_probes(pods):
    """Every near-miss class of every pod IP, less the ones that are pods themselves."""
    p = pods.ips.astype(np.uint32)
    probes = np.unique(np.concatenate([f(p) for _, f in IC.MUTATIONS]).astype(np.uint32))
    return probes[~np.isin(probes, p)]


# (three prefixes with holes are 3 * 198 blocks: too many for the dense image, as "too-wide")
IMAGE_SETS = [((1, "holes", 120), "dense"), ((3, "holes"), "row"), ((2, "edges"), "dense"),
              ((4, "too-wide"), "row"), ((1, "too-wide"), "row"), ((4, "run"), "dense"), ((5, "run"), "cuckoo"),
              ("scattered", "cuckoo")]


def test_image_probes_near_miss(harness):  # noqa: F811
    """ipl_probe / ipr_probe / iprd_probe on the cases' pod sets: every pod IP found with its
    slot and none of the near-miss addresses -- the 100k random and neighbouring probes of
    the harness as in test_ipl_build.py, then the eight classes as listed absent probes --
    resolves to a slot; each layout builds the forms it is meant to reach."""
    sets, probes = [], []
    for key, _ in IMAGE_SETS:
        pods = IC.pods_of(key)
        sets.append([(int(ip), int(o)) for ip, o in zip(pods.ips, pods.ip_owner)])
        probes.append(_absent_probes(pods).tolist())
    res = run_sets(harness, sets, probes)
    for (key, form), ents, pr, r in zip(IMAGE_SETS, sets, probes, res):
        # (two of the eight classes are one value each, and flipped octets often land on another pod)
        assert len(pr) > 2 * len(ents)
        # the cuckoo image takes 255.255.255.255 as its empty key: the probe must still miss
        assert 0xFFFFFFFF in pr and 0 in pr
        assert r["built"] == 1 and r["found"] == len(ents) and r["absent"] > 99_000, (key, r)
        assert r["xabsent"] == 0, (key, r)
        assert r["rbuilt"] == (form != "cuckoo") and r["dbuilt"] == (form == "dense"), (key, r)
        if r["rbuilt"]:
            assert r["rfound"] == len(ents) and r["rabsent"] == 0 and r["xrabsent"] == 0, (key, r)
        if r["dbuilt"]:
            assert r["dfound"] == len(ents) and r["dabsent"] == 0 and r["xdabsent"] == 0, (key, r)
        for k in ("bytes", "rbytes", "dbytes"):
            assert r[k] <= 112 * 1024
    holes, edges, wide = res[0], res[2], res[3]
    assert holes["dnblk"] == 198  # third octets 3..200, the gaps as empty blocks
    assert edges["dnblk"] == 6 and edges["nblk"] == 6  # 0..2 and 253..255
    assert wide["nblk"] == 4 * 16 and wide["npfx"] == 4


def test_host_radix_mirror_prefix_boundaries():
    """The CPU backend's IP table at 8 / 9 and 64 / 65 prefixes resolves every pod IP to its
    pod and every near-miss address to none: enriched-flow slots against a dict."""
    for npfx in (8, 9, 64, 65):
        pods, recs, _ = IC.inputs((npfx, "run"))
        g = IC.make_case_engine(pods, W.LOCAL_FWD_DROP, False, 0, None)
        try:
            slot_of = {}
            for ep in pods.endpoints:
                own = ep.owner_refs[0] if ep.owner_refs else (None, None)
                slot_of[int(ep.ips[0])] = g.slot_intern(ep.namespace, ep.name, own[0], own[1])
            hb = g.alloc_batch(len(recs))
            hb.fill(recs, 0, len(recs))
            s, d = g.submit_enrich(hb, len(recs))
        finally:
            g.close()
        for got, col in ((s, recs.src_ip), (d, recs.dst_ip)):
            want = np.array([slot_of.get(int(x), -1) for x in col], np.int32)
            np.testing.assert_array_equal(np.asarray(got[:len(recs)]), want)
            assert (want >= 0).any() and (want < 0).any()


def test_hll_cases_cpu_backend():
    """The inputs of test_hll_sources_near_miss on the host mirror of the sketch pass."""
    from . import sketch_cases as SC
    for _, key, flags, unaligned, _ in IC.HLL_CASES:
        pods, recs = IC.hll_inputs(key, unaligned)
        SC.run(SC.Backend(None), pods, [recs], 0, 0, 8, flags, None, unaligned=unaligned, sparse_capacity_log2=16)
