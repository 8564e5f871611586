"""The aggregation launch planner (retina_amd/csrc/gpuagg_launch_plan.h), compiled host-only
with g++: kernel selection, LDS and list geometry and the defer / accumulate policy, asserted
against tests/dense_cases.py's restatement (`geometry`, `kernel_name`, `spill_cap`, ...) for
every plan the dense cases run, and at the exact limits that restatement keeps MARGIN bins away
from.  No expected value comes from the planner: they are dense_cases' or literals with their
arithmetic beside them."""

import pytest

from retina_amd import workloads as W

from . import dense_cases as D
from . import host_programs

CUS = 256
LDS = D.LDS_BYTES                       # 163,840
EXTRA2 = D.LDS_EXTRA_WORDS * 8          # tier 2: 64 dummies + 128 words of spill counters: 1,536 bytes
HOT_KEYS, HOT_KEY_BYTES = 2048, 48      # kHotKeys, kHotKeyBytes
MAX_SEG_LISTS = 4096                    # kSparseMaxSegLists
WIDE_SEG_LOG2 = 12                      # kWideSegLog2
FWD, DROP, FLAGS, RETRANS, DNS_REQ, DNS_RESP = range(6)
COLS = 63                               # every column aligned
NO_BUDGET = (1 << 63) - 1               # wide lists: ~0ull >> 1


@pytest.fixture(scope="module")
def planner():
    return host_programs.planner()


def grp(fam, nbins=0, base=0, sparse=False, nsub=1, keyed=True):
    return "g=%d:%d:%d:%d:%d:%d" % (fam, sparse, nsub, base, keyed, nbins)


def dense_groups(*sizes):
    """(family, nbins[, nsub]) dense groups laid out back to back; -> (words, dense_len)."""
    out, base = [], 0
    for fam, nbins, *nsub in sizes:
        out.append(grp(fam, nbins, base, nsub=nsub[0] if nsub else 1))
        base += nbins
    return out, base


def case(groups, **facts):
    return " ".join(list(groups) + ["%s=%d" % (k.replace("__", "."), int(v)) for k, v in facts.items()])


plan = host_programs.plan


def one(exe, groups, **facts):
    return plan(exe, [case(groups, **facts)])[0]


def sig_of(*nibbles):
    return sum(n << (4 * i) for i, n in enumerate(nibbles))


# ---- agreement with dense_cases.geometry / kernel_name ---------------------------------------
def dense_case_plans():
    """(id, spec, pods, flags) of every geometry the dense cases run."""
    out = []
    for pid, (spec_id, n_pods, _, _) in D.PLANS.items():
        for flags in (0, D.NO_LDS_IP) if pid in D.PLANS_TIER1 else (0,):
            out.append((pid, D.SPECS[spec_id], D.pods_of(n_pods), flags))
    for pid in D.PLANS_KIP:
        for flags in (D.CUCKOO, D.ROW_RADIX):
            out.append((pid, D.SPECS[D.PLANS[pid][0]], D.pods_of(D.PLANS[pid][1]), flags))
    for tier, (n_pods, flags) in D.ONE_WINDOW.items():
        out.append(("one-window-" + tier, D.FWD_FLAGS_RETRANS, D.pods_of(n_pods), flags))
    out.append(("partial-window", D.DROP_ONLY, D.pods_of(D.PARTIAL_PODS), 0))
    for which, n_pods in D.BOUNDARY.items():
        out.append(("boundary-" + which, D.SIX, D.pods_of(n_pods), 0))
    out.append(("c5-no-rings", W.C5_SPEC, D.pods_of(D.NO_RINGS_PODS), 0))
    out.append(("reconcile-four", D.FOUR, D.pods_of(3000), 0))  # state_reconcile's other specs
    out.append(("reconcile-six", D.SIX, D.pods_of(3000), 0))
    for p in D.STATE_PLANS:  # state_relayout: 100 more pods
        out.append(("relayout-" + p, D.SPECS[D.PLANS[p][0]], D.state_inputs(p)[1], 0))
    return out


def test_planner_agrees_with_the_dense_cases(planner):
    """tier1, L, sig, nwin, dense_ng, dns_compact, the spill cap (deferred and per batch) and the
    name, with 256 CUs, aligned and unaligned columns.  The facts a ctx would hold: the local
    image whenever build_lds_image builds one (its form by flag, the largest size of
    ipl_bytes_range: geometry() has asserted that every size decides alike), and for a DNS plan
    helpers.make_engine's compact table of 2^20 slots."""
    cases, want = [], []
    for pid, spec, pods, flags in dense_case_plans():
        geo = D.geometry(spec, pods, flags)
        image = 0
        if not flags & D.NO_LDS_IP and D.image_holds(pods):
            image = D.ipl_bytes_range(pods, geo.kip)[1]
            image = image if image <= D.IPL_MAX_BYTES else 0
        groups = [grp(g.fam, g.nbins, g.base, g.sparse, g.nsub, g.keyed) for g in geo.groups]
        for vec in (True, False):
            for m in (10_000, 1 << 20):
                for defer in (1, 0):
                    cases.append(case(groups, dense_len=geo.dense_len, need_dns=geo.dns, compact=geo.dns,
                                      sparse_slots=(1 << D.SPARSE_CAPACITY_LOG2) if geo.dns else 0,
                                      img_local__bytes=image, img_local__form=geo.kip, m=m,
                                      aligned=COLS if vec else COLS & ~4, defer_folds=defer))
                    want.append((pid, flags, geo, vec, m, defer))
    for r, (pid, flags, geo, vec, m, defer) in zip(plan(planner, cases), want):
        what = (pid, flags, vec, m, defer, r)
        assert r["tier1"] == geo.tier1 and r["lds_bins"] == geo.L and r["nwin"] == geo.nwin, what
        assert r["dense_ng"] == next(x for x in (1, 2, 4, 8) if len(geo.groups) <= x), what
        assert r["dns_compact"] == geo.dns and r["sp_nwin"] == geo.seg_lists, what
        if geo.tier1 or not geo.dns or geo.dense():
            assert r["sig"] == geo.sig, what
        else:  # DNS groups alone: geometry() leaves the signature out; sig_group(DNS_REQ / DNS_RESP, not in LDS) = 5 / 6
            assert r["sig"] == sig_of(*[g.fam + 1 for g in geo.groups]) and r["sig"] in (5, 5 | 6 << 4), what
        assert r["name"] == D.kernel_name(geo, vec) and r["vec"] == vec, what
        # one 1,024-thread workgroup per CU with dense bins, else four of 256 threads
        blocks, threads = (CUS, 1024) if geo.dense_len else (4 * CUS, 256)
        chunk = D.launch_chunk(m, blocks)
        assert r["chunk"] == chunk <= D.SMALL_LAUNCH_CHUNK and (r["blocks"], r["threads"]) == (blocks, threads), what
        if geo.nwin:
            assert r["spill_cap"] == D.spill_cap(geo, chunk, not defer), what
            assert r["win_blocks"] == D.fold_partitions(geo, blocks)[0] * geo.nwin and r["win_shift"] == 13, what
        assert r["defer"] == (bool(defer) and bool(geo.nwin or geo.seg_lists)), what
        assert r["kip"] == (geo.kip if geo.tier1 else -1), what


def test_image_decided_by_the_largest_installed_slot(planner):
    """300 pods, 65,600 slots interned: with the largest installed id 0xFFFE build_lds_image still
    builds the local image and the plan is tier 1; with 0xFFFF (kIplNoSlot) there is none, whatever
    the number of pods.  145 spill windows either way (65,600 x 18 bins, no group fits LDS)."""
    pods = D.pods_of(300)
    assert D.image_holds(pods) and D.image_holds(pods, 0xFFFE) and not D.image_holds(pods, 0xFFFF)
    for max_slot, tier1 in ((0xFFFE, True), (0xFFFF, False)):
        geo = D.geometry(D.FWD_DROP, pods, n_slots=65_600, max_slot=max_slot)
        assert geo.tier1 == tier1 and geo.dense_len == 65_600 * 18 and (geo.L, geo.nwin) == (0, 145)
        image = D.ipl_bytes_range(pods, geo.kip)[1] if tier1 else 0
        groups = [grp(g.fam, g.nbins, g.base, g.sparse, g.nsub, g.keyed) for g in geo.groups]
        r = one(planner, groups, dense_len=geo.dense_len, img_local__bytes=image, img_local__form=geo.kip, m=10_000)
        assert (r["tier1"], r["lds_bins"], r["nwin"], r["name"]) == (tier1, 0, 145, D.kernel_name(geo)), r
        assert r["name"] == ("dense_lds_kernel<2, true, 0u, 2>" if tier1 else "dense_local_kernel<2, true, false, 0u>")


# ---- the edges the margin hides ----------------------------------------------------------------
def test_tier1_prefix_ends_at_the_limit(planner):
    """A group ending exactly at (kLdsBytes - image - kL4ExtraBytes) / 4 stays, one bin more spills
    whole: image 4,096 B -> (163,840 - 4,096 - 1,280) / 4 = 39,616 bins, and the kernel's LDS
    is then all 160 KiB."""
    limit = (LDS - 4096 - D.L4_EXTRA_BYTES) // 4
    assert limit == 39_616
    for nbins, L, sig, nwin in ((limit, limit, 9, 0), (limit + 1, 0, 1, 5)):  # sig_group(FWD, in LDS) = 1 | 8
        r = one(planner, [grp(FWD, nbins)], dense_len=nbins, img_local__bytes=4096, img_local__form=2, m=1 << 20)
        assert (r["tier1"], r["lds_bins"], r["sig"], r["nwin"]) == (1, L, sig, nwin), r
        assert r["name"] == "dense_lds_kernel<1, true, %du, 2>" % (9 if L else 0), r
        assert r["lds_bytes"] == 4096 + 4 * L + D.L4_EXTRA_BYTES and r["stage_stride"] == L, r
    assert 4096 + 4 * limit + D.L4_EXTRA_BYTES == LDS


def test_tier2_prefix_ends_at_the_limit(planner):
    """kLdsMaxBins = 20,288 u64 bins with no lists; 128 segment lists take (128 + 1) / 2 = 64
    words of them: 20,224."""
    assert D.TIER2_MAX_BINS == 20_288
    for nbins, L in ((20_288, 20_288), (20_289, 0)):
        r = one(planner, [grp(FWD, nbins)], dense_len=nbins, m=1 << 20)
        assert (r["tier1"], r["lds_bins"], r["name"]) == (0, L, "dense_local_kernel<1, true, false, 0u>"), r
        assert r["lds_bytes"] == (L + D.LDS_EXTRA_WORDS) * 8, r
    dns = dict(need_dns=1, compact=1, sparse_slots=1 << 20)
    for nbins, L in ((20_224, 20_224), (20_225, 0)):
        r = one(planner, [grp(FWD, nbins), grp(DNS_REQ, sparse=True)], dense_len=nbins, m=1 << 20, **dns)
        assert (r["dns_compact"], r["sp_nwin"], r["lds_bins"]) == (1, 128, L), r
        assert r["sig"] == sig_of(9 if L else 1, 5) and r["name"] == "dense_local_kernel<2, true, true, 0u>", r
        assert r["lds_bytes"] == (L + D.LDS_EXTRA_WORDS) * 8 + 128 * 4, r


def test_image_that_leaves_no_room(planner):
    """tier 1 needs image + kL4ExtraBytes < kLdsBytes, strictly: 162,560 B refuses, 16 B less
    leaves (163,840 - 162,544 - 1,280) / 4 = 4 bins."""
    full = LDS - D.L4_EXTRA_BYTES
    assert full == 162_560
    r = one(planner, [grp(FWD, 4)], dense_len=4, img_local__bytes=full - 16, img_local__form=1, m=4096)
    assert (r["tier1"], r["lds_bins"], r["name"], r["lds_bytes"]) == (1, 4, "dense_lds_kernel<1, true, 9u, 1>", LDS), r
    r = one(planner, [grp(FWD, 5)], dense_len=5, img_local__bytes=full - 16, img_local__form=1, m=4096)
    assert (r["tier1"], r["lds_bins"], r["nwin"]) == (1, 0, 1), r
    r = one(planner, [grp(FWD, 4)], dense_len=4, img_local__bytes=full, img_local__form=1, m=4096)
    assert (r["tier1"], r["lds_bins"], r["image"], r["name"]) == (0, 4, 0, "dense_local_kernel<1, true, false, 0u>"), r


def test_spill_windows_256_and_257(planner):
    """256 windows of 8,192 bins get lists (two fold partitions each at 256 CUs), one bin more
    gets none."""
    r = one(planner, [grp(DROP, 256 * 8192, nsub=8)], dense_len=256 * 8192, m=1 << 20)
    assert (r["lds_bins"], r["nwin"], r["win_blocks"], r["defer"], r["row_masks"]) == (0, 256, 512, 1, 1), r
    assert r["spill_cap"] == 2 * (64 * 4096) // 256 + 4096 == 6144, r  # budget 64 launches of chunk 4,096
    r = one(planner, [grp(DROP, 256 * 8192 + 1, nsub=8)], dense_len=256 * 8192 + 1, m=1 << 20)
    assert (r["lds_bins"], r["nwin"], r["spill_cap"], r["defer"], r["row_masks"]) == (0, 0, 0, 0, 0), r


def test_spill_cap_below_and_at_2_24(planner):
    """The kernels' 24-bit index math: lists only while their capacity is below 2^24.  One window,
    an accumulating launch takes the pending budget: cap = 2 * budget + 4096, so budget
    8,386,558 gives 2^24 - 4 and 8,386,560 gives 2^24 (no lists, nothing to defer)."""
    (groups, n), L = dense_groups((FWD, D.TIER2_MAX_BINS), (DROP, 8192, 8)), D.TIER2_MAX_BINS  # the drops: one window
    pend = dict(pend__active=1, pend__blocks=CUS, pend__lds_bins=L, pend__dense_len=n, pend__same_state=1, pend__rpb=4096)
    below = (1 << 24) - 4
    assert 2 * 8_386_558 + 4096 == below and 2 * 8_386_560 + 4096 == 1 << 24
    r = one(planner, groups, dense_len=n, m=1 << 20, pend__budget=8_386_558, pend__nwin=1, pend__spill_cap=below,
            pend__win_blocks=512, pend__win_shift=13, **pend)
    assert (r["lds_bins"], r["accum"], r["budget"], r["nwin"], r["spill_cap"], r["defer"]) == (L, 1, 8_386_558, 1, below, 1), r
    r = one(planner, groups, dense_len=n, m=1 << 20, pend__budget=8_386_560, **pend)
    assert (r["lds_bins"], r["accum"], r["nwin"], r["spill_cap"], r["defer"]) == (L, 1, 0, 0, 0), r


def test_small_launch_chunk(planner):
    """Spill-only plans defer at chunks of at most 2^16 records: 2^24 records on 256 workgroups.
    Deferred, the lists are sized for min(kMaxRecordsPerBlock, 64 * chunk) = 2^20 - 4 records."""
    groups, n = dense_groups((FWD, 6400), (DROP, 48_000, 8))
    facts = dict(dense_len=n, img_local__bytes=8192, img_local__form=2)
    assert (LDS - 8192 - D.L4_EXTRA_BYTES) // 4 == 38_592 and -(-48_000 // 8192) == 6
    small = r = one(planner, groups, m=1 << 24, **facts)
    assert (r["chunk"], r["defer"], r["stage_defer"], r["budget"]) == (65_536, 1, 1, (1 << 20) - 4), r
    assert r["spill_cap"] == (2 * ((1 << 20) - 4) // 6 + 4096 + 3) & ~3 == 353_620, r
    r = one(planner, groups, m=(1 << 24) + 1, **facts)
    assert (r["chunk"], r["defer"], r["stage_defer"], r["budget"]) == (65_540, 0, 0, 65_540), r
    assert r["spill_cap"] == (2 * 65_540 // 6 + 4096 + 3) & ~3 == 25_944, r
    for x in (small, r):
        assert (x["lds_bins"], x["sig"], x["nwin"], x["name"]) == (6400, 41, 6, "dense_lds_kernel<2, true, 41u, 2>"), x


REMOTE = dict(local=0, remote=1, sparse_slots=1 << 20, seg_log2=WIDE_SEG_LOG2, wide_list_bytes=32 << 30)
WIDE_SEGS = (1 << 20) >> WIDE_SEG_LOG2  # 256 lists; their counters: (256 + 1) / 2 u64 words = 1,024 B


def test_hot_cache_size(planner):
    """~chunk / 8 entries, 256 .. 2,048: doubled while entries * 16 <= chunk."""
    for chunk, hot_n in ((4092, 256), (4096, 512), (8192, 1024), (16_380, 1024), (16_384, 2048), ((1 << 20) - 4, 2048)):
        r = one(planner, [grp(FWD, sparse=True)], m=chunk * CUS, **REMOTE)
        assert (r["chunk"], r["hot"], r["hot_n"], r["v_hot_n"]) == (chunk, 1, hot_n, hot_n), r
        assert (r["blocks"], r["threads"]) == (CUS, 1024), r


def test_c5_ring_upgrade_fits_exactly(planner):
    """The staged kSigC5 kernel takes nwin * (1 + kSpillRing) * 4 more bytes when they fit.  No
    real C5 plan comes near (L = 0), so the prefix and the signature are forced: (19,966 + 192) * 8
    + 128 * 4 + 4 * 129 * 4 = 163,840 fits, one more segment list (4 bytes) does not."""
    groups = [grp(FLAGS, 80_000, 0, nsub=8), grp(RETRANS, 10_000, 80_000), grp(DNS_REQ, sparse=True), grp(DNS_RESP, sparse=True)]
    L, nwin = 19_966, 4
    facts = dict(dense_len=L + nwin * 8192, need_dns=1, compact=1, m=1 << 20, force_lds_bins=L, force_sig=D.SIG_C5)
    base = (L + D.LDS_EXTRA_WORDS) * 8 + 128 * 4
    assert base + nwin * (1 + D.SPILL_RING) * 4 == LDS
    r = one(planner, groups, sparse_slots=128 << 13, **facts)
    assert (r["nwin"], r["sp_nwin"], r["staged"], r["lds_bytes"]) == (nwin, 128, 1, LDS), r
    assert r["name"] == "dense_local_kernel<4, true, true, 25923u, true>", r
    r = one(planner, groups, sparse_slots=129 << 13, **facts)
    assert (r["nwin"], r["sp_nwin"], r["staged"], r["lds_bytes"]) == (nwin, 129, 0, base + 4), r
    assert r["name"] == "dense_local_kernel<4, true, true, 25923u>", r
    # unforced, the same plan: nothing in LDS, kSigC5 by itself, rings beside 11 windows
    r = one(planner, groups, sparse_slots=128 << 13, dense_len=90_000, need_dns=1, compact=1, m=1 << 20)
    assert (r["lds_bins"], r["sig"], r["nwin"], r["staged"], r["row_masks"]) == (0, D.SIG_C5, 11, 1, 1), r
    assert r["lds_bytes"] == EXTRA2 + 128 * 4 + 11 * 129 * 4, r


def test_signature_needs_at_most_8_groups(planner):
    """8 groups: dense_lds_kernel<8> and a signature of 8 nibbles (family + 1 | 8 in LDS); 9: no
    dense kernel takes them, the generic kernel runs without LDS bins' image."""
    fams = [FWD, FWD, DROP, DROP, FLAGS, FLAGS, RETRANS, RETRANS, FWD]
    groups, n = dense_groups(*[(f, 16) for f in fams[:8]])
    r = one(planner, groups, dense_len=n, img_local__bytes=4096, img_local__form=2, m=4096)
    assert (r["dense_ng"], r["tier1"], r["lds_bins"], r["name"]) == (8, 1, 128, "dense_lds_kernel<8, true, 0u, 2>"), r
    assert r["sig"] == sig_of(9, 9, 10, 10, 11, 11, 12, 12), r
    groups, n = dense_groups(*[(f, 16) for f in fams])
    r = one(planner, groups, dense_len=n, img_local__bytes=4096, img_local__form=2, m=4096)
    assert (r["dense_ng"], r["tier1"], r["sig"], r["lds_bins"], r["name"]) == (0, 0, 0, 144, "aggregate_kernel<true, false>"), r


def test_segment_list_limit(planner):
    """kSparseMaxSegLists = 4,096 compact segments still take lists ((4096 + 1) / 2 = 2,048 words
    of the LDS prefix's room); twice that: no lists, and the DNS groups leave the dense kernel."""
    groups, facts = [grp(FWD, 18_240), grp(DNS_REQ, sparse=True)], dict(dense_len=18_240, need_dns=1, compact=1, m=1 << 20)
    assert D.TIER2_MAX_BINS - 2048 == 18_240
    r = one(planner, groups, sparse_slots=MAX_SEG_LISTS << 13, **facts)
    assert (r["dns_compact"], r["sp_lists"], r["sp_nwin"], r["lds_bins"]) == (1, 1, 4096, 18_240), r
    assert r["sp_cap"] == (64 + 16 + 64 + 1) & ~1 == 144, r  # 64 * 4,096 records over 4,096 lists: 64 each, + 25 % + 64
    r = one(planner, groups, sparse_slots=2 * MAX_SEG_LISTS << 13, **facts)
    assert (r["dense_ng"], r["dns_compact"], r["sp_lists"], r["sp_nwin"], r["lds_bins"]) == (0, 0, 0, 0, 18_240), r
    assert r["name"] == "aggregate_kernel<true, false>" and r["defer"] == 0, r


def test_row_masks_need_aligned_rows(planner):
    """A spilled tcpflags group's 8-bin rows have to start a multiple of 8 behind the prefix:
    behind drops that fit no prefix (38,592 bins beside this image) and a keyless forward group."""
    for fwd_bins, want in ((16, 1), (2, 0)):
        groups, n = dense_groups((DROP, 48_000, 8), (FWD, fwd_bins), (FLAGS, 800, 8))
        r = one(planner, groups, dense_len=n, img_local__bytes=8192, img_local__form=2, m=4096)
        assert (r["tier1"], r["lds_bins"], r["nwin"], r["row_masks"]) == (1, 0, 6, want), r
    groups, n = dense_groups((FWD, 2), (FLAGS, 48_000, 8))  # the rows start right behind the prefix
    r = one(planner, groups, dense_len=n, img_local__bytes=8192, img_local__form=2, m=4096)
    assert (r["lds_bins"], r["nwin"], r["row_masks"]) == (2, 6, 1), r


# ---- wide_kernel ---------------------------------------------------------------------------
CACHE = HOT_KEYS * HOT_KEY_BYTES                           # 98,304 B
WIDE_LDS = 1024 + CACHE                                    # counters + cache: 99,328 B, door 2^18 bits: +32,768
GENERIC_LDS = EXTRA2 + WIDE_SEGS * 4 + 4 + CACHE           # aggregate_kernel with the cache: 100,868 B


def sparse(*fams):
    return [grp(f, sparse=True) for f in fams]


def test_wide_kernel_eligibility(planner):
    """Sparse-only plans of 1 .. 4 groups without tcpflags on the wide-key list path, vector
    loads; the doorkeeper takes the largest of 2^13 .. 2^18 bits that fit."""
    big = dict(m=1 << 24, **REMOTE)
    for fams, name in (((FWD,), "wide_kernel<2, true, true, -1>"), ((FWD, DROP), "wide_kernel<2, true, true, -1>"),
                       ((FWD, DROP, RETRANS), "wide_kernel<4, true, true, -1>"),
                       ((FWD, DROP, RETRANS, DNS_REQ), "wide_kernel<4, true, true, -1>"),
                       ((FWD, FWD), "wide_kernel<2, true, false, -1>"),
                       ((FWD, DROP, RETRANS, DROP), "wide_kernel<4, true, false, -1>")):
        r = one(planner, sparse(*fams), need_dns=DNS_REQ in fams, **big)
        assert (r["name"], r["v_hot_n"], r["door_log2"], r["lds_bytes"]) == (name, 2048, 18, WIDE_LDS + (1 << 15)), r
        assert (r["fold_cond"], r["budget"], r["sp_nwin"], r["sp_cap"]) == (1, NO_BUDGET, 256, 16_384), r
    assert WIDE_LDS + (1 << 15) <= LDS < WIDE_LDS + (1 << 16)
    generic = ("aggregate_kernel<true, false>", 2048, 18, GENERIC_LDS + (1 << 15))
    for groups in (sparse(FWD, DROP, RETRANS, DNS_REQ, DNS_RESP), sparse(FWD, FLAGS)):  # 5 groups; tcpflags
        r = one(planner, groups, **big)
        assert (r["name"], r["v_hot_n"], r["door_log2"], r["lds_bytes"]) == generic, r
    # a dense group: in LDS before the cache (limit 20,288 - 128 - (98,304 / 8 + 1) = 7,871 bins)
    # -- that prefix leaves 4 bytes, no doorkeeper; 128 bins less leave 1,028: 2^13 bits
    r = one(planner, [grp(FWD, 7871)] + sparse(DROP), dense_len=7871, **big)
    assert (r["name"], r["lds_bins"], r["door_log2"], r["lds_bytes"]) == (generic[0], 7871, 0, GENERIC_LDS + 7871 * 8), r
    assert GENERIC_LDS + 7871 * 8 == LDS - 4
    r = one(planner, [grp(FWD, 7743)] + sparse(DROP), dense_len=7743, **big)
    assert (r["name"], r["lds_bins"], r["door_log2"], r["lds_bytes"]) == (generic[0], 7743, 13, LDS - 4), r
    r = one(planner, [grp(FWD, 7872)] + sparse(DROP), dense_len=7872, **big)
    assert (r["name"], r["lds_bins"], r["nwin"]) == (generic[0], 0, 1), r
    # unaligned bytes column
    r = one(planner, sparse(FWD, DROP), **dict(big, aligned=COLS & ~4))
    assert (r["name"], r["door_log2"], r["lds_bytes"]) == ("aggregate_kernel<false, false>", 18, generic[3]), r
    # an unaligned column no group reads does not matter; count-min reads the ports
    assert one(planner, sparse(FWD), **dict(big, aligned=COLS & ~48))["name"] == "wide_kernel<2, true, true, -1>"
    assert one(planner, sparse(FWD), **dict(big, aligned=COLS & ~16, cms=1))["name"] == "aggregate_kernel<false, false>"
    # compact keys: no cache, no doorkeeper; 128 segment lists of 2^13 slots
    r = one(planner, sparse(DNS_REQ), **dict(big, compact=1, seg_log2=13, need_dns=1))
    assert (r["name"], r["hot"], r["v_hot_n"], r["door_log2"]) == ("aggregate_kernel<true, false>", 0, 0, 0), r
    assert (r["sp_nwin"], r["lds_bytes"], r["blocks"], r["threads"]) == (128, EXTRA2 + 128 * 4, 4 * CUS, 256), r
    # local context with ip / port options: wide keys, never the image
    r = one(planner, sparse(FWD, DROP), **dict(big, local=1, remote=0, img_all__bytes=4096, img_all__form=2))
    assert (r["name"], r["image"], r["door_log2"], r["lds_bytes"]) == ("wide_kernel<2, false, true, -1>", 0, 18, WIDE_LDS + (1 << 15)), r
    # the flags that take the path away
    assert one(planner, sparse(FWD), **dict(big, no_hot_keys=1))["name"] == "aggregate_kernel<true, false>"
    r = one(planner, sparse(FWD), **dict(big, no_wide_lists=1))
    assert (r["name"], r["sp_nwin"], r["hot_n"], r["door_log2"], r["fold_cond"]) == ("aggregate_kernel<true, false>", 0, 2048, 0, 0), r


def test_wide_kernel_image_fit(planner):
    """Remote context: the all-pods image beside 2,048 entries, the counters and a 2^13-bit
    doorkeeper: image + 1,024 + 98,304 + 1,024 <= 163,840, so 63,488 B fit (the doorkeeper stays
    at 2^13 bits) and 16 B more do not (no image, 2^18 bits)."""
    fit = LDS - 1024 - CACHE - 1024
    assert fit == 63_488 and fit % 16 == 0
    for form in (0, 1, 2):
        r = one(planner, sparse(FWD, DROP), m=1 << 24, img_all__bytes=fit, img_all__form=form, **REMOTE)
        assert (r["name"], r["image"], r["v_hot_n"], r["door_log2"], r["lds_bytes"]) == (
            "wide_kernel<2, true, true, %d>" % form, 2, 2048, 13, LDS), r
    r = one(planner, sparse(FWD, DROP), m=1 << 24, img_all__bytes=fit - 15, img_all__form=2, **REMOTE)  # rounded up to 16
    assert (r["kip"], r["lds_bytes"]) == (2, LDS), r
    r = one(planner, sparse(FWD, DROP), m=1 << 24, img_all__bytes=fit + 16, img_all__form=2, **REMOTE)
    assert (r["name"], r["image"], r["v_hot_n"], r["door_log2"], r["lds_bytes"]) == (
        "wide_kernel<2, true, true, -1>", 2, 2048, 18, WIDE_LDS + (1 << 15)), r
    # a small launch's smaller cache leaves the image more room: chunk 4,096 -> 512 entries
    r = one(planner, sparse(FWD, DROP), m=1 << 20, img_all__bytes=fit + 16, img_all__form=2, **REMOTE)
    assert (r["hot_n"], r["v_hot_n"], r["kip"], r["door_log2"]) == (512, 512, 2, 18), r
    assert r["lds_bytes"] == fit + 16 + 1024 + 512 * HOT_KEY_BYTES + (1 << 15), r


# ---- accumulation ----------------------------------------------------------------------------
def test_accumulation(planner):
    """A pending launch of equal geometry takes this one while rpb + chunk <= budget; another
    blocks, prefix, dense_len, list geometry or state refuses; the staged copies continue only
    from copies of the same stride."""
    groups, n = dense_groups((FWD, 6400), (DROP, 48_000, 8))
    facts = dict(dense_len=n, img_local__bytes=8192, img_local__form=2, m=1 << 20)
    chunk, budget = 4096, 64 * 4096
    cap = (2 * budget // 6 + 4096 + 3) & ~3
    assert cap == 91_480
    alone = one(planner, groups, **facts)
    assert (alone["chunk"], alone["budget"], alone["nwin"], alone["spill_cap"], alone["win_blocks"]) == (chunk, budget, 6, cap, 6 * 85), alone
    assert (alone["defer"], alone["accum"], alone["stage_defer"], alone["stage_accum"], alone["stage_stride"]) == (1, 0, 1, 0, 6400), alone
    pend = dict(pend__active=1, pend__nwin=6, pend__spill_cap=cap, pend__win_blocks=510, pend__win_shift=13,
                pend__budget=budget, pend__rpb=budget - chunk, pend__blocks=CUS, pend__lds_bins=6400, pend__dense_len=n,
                pend__same_state=1, pend__staged=1, pend__stage_stride=6400)
    r = one(planner, groups, **facts, **pend)
    assert (r["accum"], r["stage_accum"], r["budget"], r["spill_cap"], r["defer"]) == (1, 1, budget, cap, 1), r
    for change in (dict(pend__rpb=budget - chunk + 4), dict(pend__blocks=CUS - 1), dict(pend__lds_bins=6404),
                   dict(pend__dense_len=n + 8), dict(pend__spill_cap=cap + 4), dict(pend__nwin=7), dict(pend__win_blocks=504),
                   dict(pend__sp_nwin=128), dict(pend__same_state=0)):
        r = one(planner, groups, **facts, **dict(pend, **change))
        assert (r["accum"], r["stage_accum"], r["budget"], r["defer"], r["stage_defer"]) == (0, 0, budget, 1, 1), (change, r)
    for change in (dict(pend__staged=0), dict(pend__stage_stride=6404)):
        r = one(planner, groups, **facts, **dict(pend, **change))
        assert (r["accum"], r["stage_accum"], r["stage_defer"]) == (1, 0, 1), (change, r)
    # a pending budget of another chunk size is kept while the geometry is its own
    half = dict(pend, pend__budget=budget // 2, pend__spill_cap=(2 * (budget // 2) // 6 + 4096 + 3) & ~3, pend__rpb=chunk)
    r = one(planner, groups, **facts, **half)
    assert (r["accum"], r["budget"], r["spill_cap"]) == (1, budget // 2, 47_788), r
    # folds per batch (gpuagg_config: FLAG_FOLD_PER_BATCH): nothing defers, nothing accumulates
    r = one(planner, groups, **facts, **dict(pend, defer_folds=0))
    assert (r["accum"], r["defer"], r["stage_defer"], r["budget"], r["spill_cap"]) == (0, 0, 0, chunk, (2 * chunk // 6 + 4096 + 3) & ~3), r


def test_wide_lists_have_no_budget(planner):
    """Wide lists: folded when the device says so, so the budget is unbounded, the capacity comes
    from wide_list_bytes (32 GiB / 32 B / (256 workgroups * 256 lists); narrow entries: 24 B) and
    any pending launch of the same geometry accumulates."""
    facts = dict(m=1 << 20, **REMOTE)
    r = one(planner, sparse(FWD, DROP), **facts)
    assert (r["fold_cond"], r["defer"], r["budget"], r["sp_nwin"], r["sp_cap"]) == (1, 1, NO_BUDGET, 256, (32 << 30) // 32 // (256 * 256)), r
    assert r["sp_cap"] == 16_384
    n = one(planner, sparse(FWD, DROP), **dict(facts, narrow=1))
    assert n["sp_cap"] == ((32 << 30) // 24 // (256 * 256)) & ~1 == 21_844, n
    pend = dict(pend__active=1, pend__sp_nwin=256, pend__sp_cap=16_384, pend__budget=NO_BUDGET, pend__rpb=1 << 40,
                pend__blocks=CUS, pend__same_state=1)
    r = one(planner, sparse(FWD, DROP), **facts, **pend)
    assert (r["accum"], r["fold_cond"], r["budget"]) == (1, 1, NO_BUDGET), r
    r = one(planner, sparse(FWD, DROP), **dict(facts, defer_folds=0))
    assert (r["fold_cond"], r["defer"], r["budget"], r["sp_cap"]) == (0, 0, 4096, 16_384), r
    # compact lists (no LDS state: 1,024 workgroups): 64 launches of 1,024 records over 128 lists + 25 % + 64
    r = one(planner, sparse(DNS_REQ), **dict(facts, compact=1, seg_log2=13, need_dns=1))
    assert (r["fold_cond"], r["defer"], r["budget"], r["sp_cap"]) == (0, 1, 64 * 1024, 512 + 128 + 64), r
