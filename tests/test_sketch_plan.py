"""The sketch launch planner (retina_amd/csrc/gpuagg_sketch_plan.h), compiled host-only with g++:
list geometry and capacities, the scatter kernel with its rings and LDS, the fold shapes and the
defer / accumulate policy, asserted against the restatements the GPU cases already keep --
sketch_cases.list_geometry / stage / scatter, slot_range_cases.hll_shape -- for every shape
those cases run, against a restatement of stage_words below, and at the limits no GPU case
reaches.  No expected value comes from the planner: they are the restatements' or literals with
their arithmetic beside them."""

import pytest

from . import dense_cases as D
from . import host_programs
from . import sketch_cases as K
from . import slot_range_cases as R

CUS = 256
LDS = D.LDS_BYTES                    # 163,840
DEFER = 1 << 22                      # kSketchDeferRecords
PER_LAUNCH = CUS << 20               # at most 2^20 records per scatter workgroup and launch
COLS = 63                            # every column aligned
UNALIGNED = COLS & ~1                # the source column 4 bytes off
CUCKOO_FORM, ROW_FORM, DENSE_FORM = 0, 1, 2  # LdsImageFacts::form; sketch_stage_kernel's kIp is form + 1


@pytest.fixture(scope="module")
def planner():
    return host_programs.sketch_planner()


def case(**facts):
    return " ".join("%s=%d" % (k.replace("__", "."), int(v)) for k, v in facts.items())


def one(exe, **facts):
    return host_programs.plan(exe, [case(**facts)])[0]


# ---- restatements ---------------------------------------------------------------------------
def ring(mean: int) -> int:
    """A staging ring: 1.5 x a round's mean appends + 64, rounded up to a power of two."""
    r = 64
    while r < mean + mean // 2 + 64:
        r <<= 1
    return r


def stage_bytes(d: int, nwin: int, hnsup: int, rnd: int, image: int):
    """sketch_stage_kernel's LDS at `rnd` records per lane and round (1,024 lanes): stage_words
    -- rc, rb per window and hc, hb per super-window; the u16 rings and one dummy u32; the u32
    rings and 64 dummies, each part rounded up to 16 bytes -- times 4, plus the IP image.
    -> (bytes, sbc, sbh)"""
    sbc = ring(1024 * rnd * d // nwin) if nwin else 0
    sbh = ring(1024 * rnd // hnsup) if hnsup else 0
    words = ((2 * (nwin + hnsup) + 3) & ~3) + ((nwin * sbc // 2 + 1 + 3) & ~3) + hnsup * sbh + 64
    return 4 * words + image, sbc, sbh


def geom(d: int, w: int, p: int, slots: int, cus: int = CUS):
    """The geometry by sketch_cases.list_geometry / slot_range_cases.hll_shape (chunk and the
    capacities are those of one 4,096-record-per-workgroup launch and not used), with the fold
    workgroups beside them: whole multiples of nwin up to one per CU, and CUs / hnsup split
    workgroups per super-window, 1 .. 64."""
    g = dict(win_shift=0, nwin=0, fold_blocks=0, hll_shift=0, hll_sshift=0, hll_nwin=0, hll_nsup=0, hll_b2=0)
    if d:
        lg = K.list_geometry(4096 * cus, cus, d, w, 10, 1)
        g.update(win_shift=lg["win_shift"], nwin=lg["nwin"], fold_blocks=lg["nwin"] * max(1, cus // lg["nwin"]))
    else:
        g["win_shift"] = min(15, w)
    if p:
        hs = R.hll_shape(p, slots, 4096 * cus, cus)
        assert hs["lists"]
        g.update(hll_shift=hs["hshift"], hll_sshift=hs["hsshift"], hll_nwin=hs["hnwin"], hll_nsup=hs["hnsup"],
                 hll_b2=min(64, max(1, cus // hs["hnsup"])))
    return g


def pend(g, **kw):
    """An active waiting set of geometry g, sized for the deferral budget, one launch in."""
    facts = dict(pend__active=1, pend__budget=DEFER, pend__rpb=4096, pend__blocks=CUS, pend__same_state=1)
    facts.update({"pend__" + k: v for k, v in g.items()})
    facts.update(kw)
    return facts


def assert_geom(r, g, what):
    assert {k: r[k] for k in g} == g, what


# ---- agreement with sketch_cases --------------------------------------------------------------
def sketch_case_shapes():
    """(id, d, w, p, flags, pods, n, unaligned, name) of every shape the sketch cases run."""
    out = []
    for d, flags in K.DEPTHS + [(4, 0)]:
        name = K.stage(flags, d, 10) if d <= K.STAGE_MAX_DEPTH else K.scatter(True, flags)
        out.append(("depth%d-f%d" % (d, flags), d, 12, 10, flags, 100, 60_000, False, name))
    for d in (4, 3):
        out.append(("cms_only%d" % d, d, 16, 0, 0, 100, 100_000, False, K.stage(0, d, 0)))
    for p, n_pods in K.HLL_ONLY:
        out.append(("hll_only%d" % p, 0, 0, p, 0, n_pods, 100_000, False, K.stage(0, 0, p)))
    for w in K.NARROW:
        out.append(("narrow%d" % w, 4, w, 10, 0, 100, 100_000, False, K.stage(0, 4, 10)))
    for flags in (0, K.CUCKOO):
        out.append(("rings_do_not_fit-f%d" % flags, 5, 22, 10, flags, 100, 100_000, False, K.scatter(True, flags)))
    out.append(("direct_hll", 4, 12, 18, 0, 64, 100_000, False, K.scatter(True, 0)))
    out.append(("direct_flag", 3, 12, 10, K.DIRECT, 100, 100_000, False, K.scatter(True, K.DIRECT)))
    for d, flags in K.UNALIGNED:
        out.append(("unaligned%d-f%d" % (d, flags), d, 12, 10, flags, 100, 100_003, True, K.scatter(False, flags)))
    for un in (False, True):
        name = K.scatter(False, 0) if un else K.stage(0, K.OVERFLOW_D, K.OVERFLOW_P)
        out.append(("list_overflow-%d" % un, K.OVERFLOW_D, K.OVERFLOW_W, K.OVERFLOW_P, 0, K.OVERFLOW_PODS, K.OVERFLOW_N, un, name))
    return out


def image_facts(flags: int, n_pods: int):
    """The all-pods image a ctx of these flags holds: its form, and the least plausible and the
    largest size (dense_cases.ipl_bytes_range; + 512: the apiserver pseudo pod's block)."""
    form = CUCKOO_FORM if flags & K.CUCKOO else ROW_FORM if flags & K.ROW_RADIX else DENSE_FORM
    lo, hi = D.ipl_bytes_range(D.pods_of(n_pods), form)
    return form, (max(lo, 512) & ~15, (hi + 512 + 15) & ~15)


def test_planner_agrees_with_the_sketch_cases(planner):
    """The scatter kernel's name, and under FOLD_PER_BATCH list_geometry's chunk, windows and
    capacities, for every shape of sketch_cases at 256 CUs, both image sizes; deferred, the same
    geometry with capacities for 2^22 records per workgroup."""
    cases, want = [], []
    for cid, d, w, p, flags, n_pods, n, un, name in sketch_case_shapes():
        form, sizes = image_facts(flags, n_pods)
        slots = n_pods + 64 if p else 0
        for image in sizes:
            for defer in (0, 1):
                cases.append(case(cms_depth=d, cms_wlog2=w, hll_p=p, hll_slots=slots, direct_sketch=bool(flags & K.DIRECT),
                                  defer_folds=defer, img_all__bytes=image, img_all__form=form, n=n,
                                  aligned=UNALIGNED if un else COLS))
                want.append((cid, d, w, p, flags, slots, n, un, name, defer))
    for r, (cid, d, w, p, flags, slots, n, un, name, defer) in zip(host_programs.plan(planner, cases), want):
        what = (cid, defer, r)
        assert r["name"] == name and r["vec"] == (not un) and r["batches"] == 1 and r["scatter"] == 1, what
        assert r["staged"] == name.startswith("sketch_stage_kernel"), what
        direct = bool(flags & K.DIRECT)
        cms_lists, hll_lists = bool(d) and not direct, bool(p) and p <= 17 and not direct
        lg = K.list_geometry(n, CUS, d or 1, w, p if hll_lists else 10, slots if hll_lists else 1)
        deferred = bool(defer) and (cms_lists or hll_lists)
        assert (r["chunk"], r["defer"], r["fold_first"], r["accum"]) == (lg["chunk"], deferred, 0, 0), what
        rpb = DEFER if deferred else lg["chunk"]
        lb = K.list_geometry(rpb * CUS, CUS, d or 1, w, p if hll_lists else 10, slots if hll_lists else 1)
        assert lb["chunk"] == rpb
        if cms_lists:
            assert (r["win_shift"], r["nwin"], r["cap"]) == (lg["win_shift"], lg["nwin"], lb["cap"]), what
        else:
            assert (r["nwin"], r["cap"], r["fold_blocks"]) == (0, 0, 0), what
        if hll_lists:
            assert (r["hll_sshift"], r["hll_nsup"], r["hll_cap"]) == (lg["hsshift"], lg["hnsup"], lb["hcap"]), what
        else:
            assert (r["hll_nsup"], r["hll_nwin"], r["hll_cap"], r["hll_cap2"]) == (0, 0, 0, 0), what
        # the folds run with the batch unless it defers; side by side only from fold_pending
        assert (r["fold_cms"], r["fold_hll"]) == ((cms_lists and not deferred), (hll_lists and not deferred)), what


def test_planner_agrees_with_the_hll_row_table(planner):
    """slot_range_cases.HLL_ROWS: fine and super-windows, the level-1 capacity of its 20,000
    records under FOLD_PER_BATCH, lists or direct CAS, and the scatter kernel that follows."""
    for which, (p, interned, max_slots, lists) in R.HLL_ROWS.items():
        rows = min(interned, max_slots)
        hs = R.hll_shape(p, rows, R.HLL_N, CUS)
        assert hs["lists"] == lists
        image = 4096 if rows <= 0xFFFF else 0  # an LDS image holds u16 slots
        r = one(planner, hll_p=p, hll_slots=rows, defer_folds=0, n=R.HLL_N, img_all__bytes=image, img_all__form=DENSE_FORM)
        assert (r["hll_shift"], r["hll_sshift"], r["chunk"]) == (hs["hshift"], hs["hsshift"], hs["chunk"]), (which, r)
        if lists:
            assert (r["hll_nwin"], r["hll_nsup"], r["hll_cap"], r["fold_hll"]) == (hs["hnwin"], hs["hnsup"], hs["hcap"], 1), (which, r)
            assert r["name"] == "sketch_stage_kernel<%d, 0>" % (3 if image else 0), (which, r)
        else:
            assert (r["hll_nwin"], r["hll_nsup"], r["hll_cap"], r["fold_hll"]) == (0, 0, 0, 0), (which, r)
            assert r["name"] == "sketch_scatter_kernel<true, false>", (which, r)  # a dense radix image is not probed unstaged
    # the row counts the issue names, with their windows written out
    table = {(17, 8192): (8192, 16), (17, 8256): (0, 0), (10, 70_016): (547, 9), (10, 2112): (17, 9), (10, 2048): (16, 16)}
    assert -(-70_016 // 128) == 547 and -(-70_016 // 8192) == 9 and -(-2112 // 256) == 9 and 8192 // 512 == 16
    for (p, rows), (hnwin, hnsup) in table.items():
        r = one(planner, hll_p=p, hll_slots=rows, n=4096)
        assert (r["hll_nwin"], r["hll_nsup"]) == (hnwin, hnsup), (p, rows, r)


# ---- the limits no GPU case reaches -------------------------------------------------------------
def test_cms_windows_4096_and_4608(planner):
    """d = 8, w = 2^24: 8 * 2^(24 - 15) = 4,096 windows still take lists (one fold workgroup each);
    d = 9: 4,608 windows, every update a direct atomic from the unstaged kernel and nothing to fold;
    the submit still defers, as any count-min does (the fold at the sync then launches nothing),
    and stops deferring with FOLD_PER_BATCH."""
    assert 8 << (24 - 15) == 4096 and 9 << (24 - 15) == 4608
    r = one(planner, cms_depth=8, cms_wlog2=24, n=1 << 20)
    assert (r["win_shift"], r["nwin"], r["fold_blocks"], r["defer"], r["cms_lds"]) == (15, 4096, 4096, 1, 4 << 15), r
    assert r["cap"] == (DEFER * 8 // 4096 * 9 // 8 + 2048 + 7) & ~7 == 11_264, r  # 8,192 a list + 12.5 % + 2,048
    # 4,096 windows: the u16 rings alone are 4096 * 64 * 2 B = 512 KiB
    assert (r["staged"], r["name"]) == (0, "sketch_scatter_kernel<true, false>"), r
    assert r["lds_bytes"] == 4096 * 4, r
    r = one(planner, cms_depth=9, cms_wlog2=24, n=1 << 20)
    assert (r["nwin"], r["fold_blocks"], r["cap"], r["defer"], r["fold_cms"], r["cms_lds"]) == (0, 0, 0, 1, 0, 0), r
    assert (r["name"], r["lds_bytes"]) == ("sketch_scatter_kernel<true, false>", 0), r
    waiting = pend(geom(0, 24, 0, 0))  # such a waiting set: no lists, nothing for either fold or the heavy hitters
    r = one(planner, cms_depth=9, cms_wlog2=24, n=1 << 20, **waiting)
    assert (r["accum"], r["fold_first"], r["pend_fold_cms"], r["pend_fold_hll"], r["hh"]) == (1, 0, 0, 0, 0), r
    r = one(planner, cms_depth=9, cms_wlog2=24, n=1 << 20, defer_folds=0)
    assert (r["defer"], r["fold_cms"], r["fold_hll"]) == (0, 0, 0), r
    # the same widths with HLL lists: the count-min goes direct alone, the pass still defers
    r = one(planner, cms_depth=9, cms_wlog2=24, hll_p=10, hll_slots=100, n=1 << 20)
    assert (r["nwin"], r["hll_nsup"], r["defer"], r["name"]) == (0, 1, 1, "sketch_scatter_kernel<true, false>"), r


def windows(rows: int, shift: int) -> int:
    return -(-rows >> shift)


def hll_restated(p: int, rows: int):
    """(hshift, hsshift, hnwin, hnsup) by list_geometry's rule, for any row count."""
    hshift = min(8, 17 - p)
    ss = hshift
    while windows(rows, ss) > 16 and ss < 26 - p and ss < hshift + 10:
        ss += 1
    return hshift, ss, windows(rows, hshift), windows(rows, ss)


def test_hll_window_limits_by_enumeration(planner):
    """p = 4 .. 18 and the row counts around every power of two up to 2^32 - 1 (hll_slots is a
    u32; kMaxSlot + 1 = 2^21 - 1 rows is among them): lists exactly while hnwin <= 8,192 and
    hnsup <= 1,024.  No input has more than 1,024 super-windows with at most 8,192 fine windows:
    super-windows hold at least 2^9 fine ones before they pass 16, so hnsup > 1,024 needs
    hnwin > 2^19.  The bound is kept and this test says that nothing reaches it alone."""
    cases, want = [], []
    for p in range(4, 19):
        rows = sorted({x for s in range(0, 33) for x in ((1 << s) - 1, 1 << s, (1 << s) + 1) if 0 < x < 1 << 32}
                      | {8192 << min(8, max(0, 17 - p)), (8192 << min(8, max(0, 17 - p))) + 1, (1 << 21) - 1})
        for n_rows in rows:
            cases.append(case(hll_p=p, hll_slots=n_rows, n=4096))
            want.append((p, n_rows))
    sup_alone = []
    for r, (p, n_rows) in zip(host_programs.plan(planner, cases), want):
        if p > 17:
            assert (r["hll_nwin"], r["hll_nsup"], r["hll_shift"], r["hll_sshift"]) == (0, 0, 0, 0), (p, n_rows, r)
            continue
        hshift, ss, hnwin, hnsup = hll_restated(p, n_rows)
        lists = hnwin <= R.HLL_MAX_WINDOWS and hnsup <= 1024
        if hnsup > 1024 and hnwin <= R.HLL_MAX_WINDOWS:
            sup_alone.append((p, n_rows))
        assert (r["hll_shift"], r["hll_sshift"]) == (hshift, ss), (p, n_rows, r)
        assert (r["hll_nwin"], r["hll_nsup"]) == ((hnwin, hnsup) if lists else (0, 0)), (p, n_rows, r)
        assert r["hll_b2"] == min(64, max(1, CUS // max(1, r["hll_nsup"]))), (p, n_rows, r)
    assert not sup_alone, sup_alone
    assert len(cases) > 1000


def test_submit_of_two_batches(planner):
    """(n_cu << 20) + 1 records: a second launch inside the submit, of one record; nothing is
    deferred, each batch folds its own lists.  One record less is one deferred launch."""
    for cus in (4, 16):
        facts = dict(cms_depth=4, cms_wlog2=12, hll_p=10, hll_slots=100, n_cu=cus)
        r = one(planner, n=(cus << 20) + 1, **facts)
        assert (r["per_launch"], r["batches"], r["last_m"], r["last_chunk"], r["defer"]) == (cus << 20, 2, 1, 4, 0), r
        assert (r["chunk"], r["fold_cms"], r["fold_hll"], r["last_fold_cms"], r["last_fold_hll"]) == (1 << 20, 1, 1, 1, 1), r
        assert r["cap"] == ((1 << 20) + (1 << 17) + 2048 + 7) & ~7, r  # 4 windows: one row each, chunk entries + 12.5 % + 2,048
        r = one(planner, n=cus << 20, **facts)
        assert (r["batches"], r["last_m"], r["chunk"], r["defer"], r["fold_cms"], r["fold_hll"]) == (1, cus << 20, 1 << 20, 1, 0, 0), r
        # a waiting set is folded before a submit that cannot defer
        g = geom(4, 12, 10, 100, cus)
        r = one(planner, n=(cus << 20) + 1, **dict(facts, **pend(g, pend__blocks=cus)))
        assert (r["defer"], r["fold_first"], r["accum"], r["b_accum"]) == (0, 1, 0, 0), r


# ---- ring rounds and LDS bytes ------------------------------------------------------------------
def test_staged_rounds(planner):
    """Round 4 when stage_words' bytes and the image fit 160 KiB, else round 2, else unstaged."""
    # C3: d = 4, w = 2^20, p = 14, 10,064 rows: 128 windows, 10 super-windows of 1,024 pods
    g = geom(4, 20, 14, 10_064)
    assert (g["nwin"], g["fold_blocks"], g["hll_shift"], g["hll_sshift"], g["hll_nwin"], g["hll_nsup"], g["hll_b2"]) == (
        128, 256, 3, 10, 1258, 10, 25)
    lds, sbc, sbh = stage_bytes(4, 128, 10, 4, 43_520)
    assert (sbc, sbh) == (256, 1024) and lds == 4 * (276 + 16_388 + 10_240 + 64) + 43_520 == 151_392
    r = one(planner, cms_depth=4, cms_wlog2=20, hll_p=14, hll_slots=10_064, n=1 << 20, img_all__bytes=43_520, img_all__form=DENSE_FORM)
    assert_geom(r, g, r)
    assert (r["name"], r["round"], r["sbc"], r["sbh"], r["lds_bytes"]) == ("sketch_stage_kernel<3, 4>", 4, 256, 1024, lds), r
    # d = 8 at w <= 2^15, one HLL super-window: 8 windows; round 4: 8 * 8,192 * 2 + 8,192 * 4 B of rings
    # alone are 160 KiB, round 2: half
    for w in (4, 12, 15):
        for image in (0, 4096):
            lds4, sbc4, sbh4 = stage_bytes(8, 8, 1, 4, image)
            lds2, sbc2, sbh2 = stage_bytes(8, 8, 1, 2, image)
            assert (sbc4, sbh4, sbc2, sbh2) == (8192, 8192, 4096, 4096) and lds4 > LDS and lds2 == 4 * (20 + 16_388 + 4096 + 64) + image
            r = one(planner, cms_depth=8, cms_wlog2=w, hll_p=10, hll_slots=100, n=60_000, img_all__bytes=image, img_all__form=DENSE_FORM)
            assert (r["nwin"], r["hll_nsup"], r["staged"], r["round"], r["sbc"], r["sbh"], r["lds_bytes"]) == (8, 1, 1, 2, 4096, 4096, lds2), r
            assert r["name"] == "sketch_stage_kernel<%d, 0>" % (3 if image else 0), r
    # d = 7 there: 7 windows of ring(4,096 * 7 / 7) = 8,192 entries fit round 4 with 16 KiB to spare
    lds4, sbc4, sbh4 = stage_bytes(7, 7, 1, 4, 0)
    assert (sbc4, sbh4) == (8192, 8192) and lds4 == 4 * (16 + 28_676 + 8192 + 64) == 147_792
    r = one(planner, cms_depth=7, cms_wlog2=15, hll_p=10, hll_slots=100, n=60_000)
    assert (r["round"], r["sbc"], r["sbh"], r["lds_bytes"]) == (4, 8192, 8192, lds4), r


def test_round2_and_the_image_size(planner):
    """sketch_cases.rings_round2: d = 4, w = 2^22, one super-window: 512 windows of 128-entry rings,
    168,224 B at round 4, 151,840 B at round 2: beside an image of up to 12,000 B the staged kernel
    at round 2, beside a larger one the unstaged kernel (which probes only a cuckoo image)."""
    lds4, _, _ = stage_bytes(4, 512, 1, 4, 0)
    lds2, sbc2, sbh2 = stage_bytes(4, 512, 1, 2, 0)
    assert (lds4, lds2, sbc2, sbh2) == (168_224, 151_840, 128, 4096) and LDS - lds2 == 12_000
    facts = dict(cms_depth=4, cms_wlog2=22, hll_p=10, hll_slots=100, n=100_000)  # 100 rows: one window of 128
    for image, form, name, lds in ((0, DENSE_FORM, "sketch_stage_kernel<0, 4>", lds2),
                                   (2048, DENSE_FORM, "sketch_stage_kernel<3, 4>", lds2 + 2048),
                                   (11_984, ROW_FORM, "sketch_stage_kernel<2, 4>", LDS - 16),
                                   (12_000, CUCKOO_FORM, "sketch_stage_kernel<1, 4>", LDS),
                                   (12_016, DENSE_FORM, "sketch_scatter_kernel<true, false>", 516 * 4),
                                   (12_016, ROW_FORM, "sketch_scatter_kernel<true, false>", 516 * 4),
                                   (12_016, CUCKOO_FORM, "sketch_scatter_kernel<true, true>", 516 * 4 + 12_016)):
        r = one(planner, img_all__bytes=image, img_all__form=form, **facts)
        assert (r["nwin"], r["hll_nsup"], r["name"], r["lds_bytes"]) == (512, 1, name, lds), (image, form, r)
        assert (r["staged"], r["round"], r["sbc"], r["sbh"]) == ((1, 2, 128, 4096) if lds >= lds2 else (0, 0, 0, 0)), (image, form, r)
    # rings_do_not_fit, d = 5: 640 windows, the u16 rings alone are 640 * 128 * 2 = 163,840 B at either round
    assert stage_bytes(5, 640, 1, 2, 0)[0] > LDS
    r = one(planner, **dict(facts, cms_depth=5))
    assert (r["nwin"], r["staged"], r["name"], r["lds_bytes"]) == (640, 0, "sketch_scatter_kernel<true, false>", 644 * 4), r


def test_image_beside_the_plain_counters(planner):
    """The image is used only if it fits beside the unstaged kernel's plain counters: 4,096 + 4
    counters leave 163,840 - 16,400 = 147,440 B; 16 B more and the lookups go to the HBM table."""
    facts = dict(cms_depth=8, cms_wlog2=24, hll_p=10, hll_slots=100, n=1 << 20, img_all__form=CUCKOO_FORM)
    counters = (4096 + 1 + 3 & ~3) * 4
    assert counters == 16_400 and LDS - counters == 147_440
    r = one(planner, img_all__bytes=147_440, **facts)
    assert (r["name"], r["lds_ip"], r["lds_bytes"]) == ("sketch_scatter_kernel<true, true>", 1, LDS), r
    r = one(planner, img_all__bytes=147_456, **facts)
    assert (r["name"], r["lds_ip"], r["lds_bytes"]) == ("sketch_scatter_kernel<true, false>", 0, counters), r
    # without HLL nothing is looked up: no image, whatever its size
    r = one(planner, cms_depth=4, cms_wlog2=12, n=4096, img_all__bytes=4096, img_all__form=DENSE_FORM)
    assert (r["name"], r["lds_ip"]) == ("sketch_stage_kernel<0, 4>", 0), r


def test_fold_shapes(planner):
    """cms_fold's window, hll_fold's registers and the split kernel's rings: a round of 4,096
    entries over nfine windows, x 2 + 64 to a power of two, doubled up to 256 while
    (2 + 2R) * nfine * 4 <= 160 KiB, flushed every (R - 64) / (2 * mean) rounds."""
    # C3's 128 fine windows: 2 * 32 + 64 = 128 -> 256 entries ((2 + 256) * 128 * 4 = 132,096 B), every (256 - 64) / 64 = 3 rounds
    r = one(planner, cms_depth=4, cms_wlog2=20, hll_p=14, hll_slots=10_064, n=1 << 20, defer_folds=0)
    assert (r["sbs"], r["sbs_every"], r["split_lds"], r["hll_lds"], r["cms_lds"]) == (256, 3, 132_096, 1 << 17, 1 << 17), r
    assert r["hll_cap2"] == (((1 << 20) // (10 * 25 * 128)) * 5 // 4 + 64 + 15) & ~15 == 112, r  # 32 a list + 25 % + 64
    # p = 17, 4,096 rows: 16 super-windows of 256 one-pod windows: 2 * 16 + 64 -> 128 entries
    # ((2 + 128) * 256 * 4 = 133,120 B; 256 entries would take 264,192), every (128 - 64) / 32 = 2 rounds
    assert hll_restated(17, 4096) == (0, 8, 4096, 16)
    r = one(planner, hll_p=17, hll_slots=4096, n=1 << 20, defer_folds=0)
    assert (r["sbs"], r["sbs_every"], r["split_lds"], r["hll_lds"], r["cms_lds"]) == (128, 2, 133_120, 1 << 17, 0), r
    # 8,192 rows: 512 fine windows: 2 * 8 + 64 -> 128 entries would take (2 + 128) * 512 * 4 = 266,240 B: no rings
    assert hll_restated(17, 8192) == (0, 9, 8192, 16)
    r = one(planner, hll_p=17, hll_slots=8192, n=1 << 20, defer_folds=0)
    assert (r["sbs"], r["sbs_every"], r["split_lds"]) == (0, 1, 2 * 512 * 4), r
    # one fine window per super-window (p = 10, 2,048 rows): 2 * 4,096 + 64 -> 16,384 entries, 65,544 B
    r = one(planner, hll_p=10, hll_slots=2048, n=1 << 20, defer_folds=0)
    assert (r["sbs"], r["sbs_every"], r["split_lds"], r["hll_lds"]) == (16_384, 1, (2 + 16_384) * 4, 1 << 17), r
    # narrow rows and low precision: the window is the row, the registers 2^(p + hshift) bytes
    r = one(planner, cms_depth=4, cms_wlog2=4, hll_p=4, hll_slots=300, n=1 << 20, defer_folds=0)
    assert (r["win_shift"], r["cms_lds"], r["hll_shift"], r["hll_lds"]) == (4, 64, 8, 1 << 12), r


# ---- the defer policy ---------------------------------------------------------------------------
C3 = dict(cms_depth=4, cms_wlog2=20, hll_p=14, hll_slots=10_064)


def test_defer_bounds(planner):
    """A submit defers while it is one launch (n <= n_cu << 20).  Its chunk is then at most 2^20, so
    2 * chunk <= 2^22 = kSketchDeferRecords holds for every such submit: that bound cannot be crossed
    from either side, the launch bound decides (test_submit_of_two_batches).  Deferred lists are sized
    for the budget, per-batch ones for the chunk."""
    assert 2 * K.list_geometry(PER_LAUNCH, CUS, 4, 20, 14, 10_064)["chunk"] == 1 << 21 <= DEFER
    r = one(planner, n=PER_LAUNCH, **C3)
    assert (r["defer"], r["chunk"], r["budget"], r["batches"]) == (1, 1 << 20, DEFER, 1), r
    assert r["cap"] == (DEFER * 4 // 128 * 9 // 8 + 2048 + 7) & ~7 == 149_504, r
    assert r["hll_cap"] == (DEFER // 10 * 5 // 4 + 64 + 15) & ~15 == 524_352, r
    r = one(planner, n=PER_LAUNCH, defer_folds=0, **C3)
    assert (r["defer"], r["cap"], r["hll_cap"]) == (0, ((1 << 15) * 9 // 8 + 2048 + 7) & ~7, (104_857 * 5 // 4 + 64 + 15) & ~15), r
    r = one(planner, n=0, **C3)  # nothing to launch: nothing planned
    assert (r["batches"], r["chunk"], r["scatter"]) == (0, 0, 0), r


def test_accumulation(planner):
    """A waiting set of equal geometry takes the submit while rpb + chunk <= budget; one record per
    workgroup more, another geometry, block count or state folds it first."""
    g = geom(4, 20, 14, 10_064)
    n, chunk = 1 << 20, 4096
    r = one(planner, n=n, **C3, **pend(g, pend__rpb=DEFER - chunk))
    assert (r["defer"], r["accum"], r["b_accum"], r["fold_first"], r["budget"], r["chunk"]) == (1, 1, 1, 0, DEFER, chunk), r
    assert (r["cap"], r["hll_cap"], r["fold_cms"], r["fold_hll"]) == (149_504, 524_352, 0, 0), r
    for past in (1, 4):  # (the engine's rpb is a multiple of 4; the rule is exact to the record)
        r = one(planner, n=n, **C3, **pend(g, pend__rpb=DEFER - chunk + past))
        assert (r["defer"], r["accum"], r["b_accum"], r["fold_first"], r["budget"]) == (1, 0, 0, 1, DEFER), (past, r)
    for change in (dict(pend__blocks=CUS - 1), dict(pend__same_state=0), dict(pend__nwin=64), dict(pend__win_shift=14),
                   dict(pend__fold_blocks=128), dict(pend__hll_shift=2), dict(pend__hll_sshift=11), dict(pend__hll_nwin=1259),
                   dict(pend__hll_nsup=9), dict(pend__hll_b2=28)):
        r = one(planner, n=n, **C3, **pend(g, **change))
        assert (r["defer"], r["accum"], r["b_accum"], r["fold_first"]) == (1, 0, 0, 1), (change, r)
    # a smaller budget is kept while the submit fits it
    r = one(planner, n=n, **C3, **pend(g, pend__budget=8192, pend__rpb=4096))
    assert (r["accum"], r["budget"], r["cap"]) == (1, 8192, (8192 * 4 // 128 * 9 // 8 + 2048 + 7) & ~7), r
    # folds per batch: the waiting set (of a ctx that deferred before) is folded first
    r = one(planner, n=n, defer_folds=0, **C3, **pend(g))
    assert (r["defer"], r["accum"], r["fold_first"], r["fold_cms"], r["fold_hll"]) == (0, 0, 1, 1, 1), r
    # nothing waits: nothing to fold first
    r = one(planner, n=n, **C3)
    assert (r["defer"], r["accum"], r["fold_first"]) == (1, 0, 0), r


def test_pending_folds(planner):
    """fold_pending_sketch: both folds, side by side when both are due, the level-2 lists sized
    for every record of the waiting set.  hh_fold_cms: nothing when nothing waits or the count-min
    went direct; the count-min fold alone while HLL lists wait; the whole fold when none do."""
    NONE, CMS_ONLY, WHOLE = 0, 1, 2
    g = geom(4, 20, 14, 10_064)
    r = one(planner, n=0, **C3, **pend(g, pend__rpb=1 << 16))
    assert (r["pend_fold_cms"], r["pend_fold_hll"], r["pend_fork"]) == (1, 1, 1), r
    assert r["pend_cap2"] == (((1 << 16) * 256 // (10 * 25 * 128)) * 5 // 4 + 64 + 15) & ~15 == 720, r  # 524 a list + 25 % + 64
    assert (r["hh"], r["hh_fold_cms"], r["hh_fold_hll"], r["hh_fork"]) == (CMS_ONLY, 1, 0, 0), r
    r = one(planner, n=0, **C3)  # nothing waits
    assert r["hh"] == NONE, r
    direct_cms = dict(cms_depth=9, cms_wlog2=24, hll_p=14, hll_slots=10_064)
    g = geom(0, 24, 14, 10_064)
    r = one(planner, n=0, **direct_cms, **pend(g))
    assert (r["hh"], r["pend_fold_cms"], r["pend_fold_hll"], r["pend_fork"]) == (NONE, 0, 1, 0), r
    for p in (0, 18):  # no HLL, or HLL by direct CAS: no HLL lists wait
        g = geom(4, 20, 0, 0)
        r = one(planner, n=0, cms_depth=4, cms_wlog2=20, hll_p=p, hll_slots=64 if p else 0, **pend(g))
        assert (r["hh"], r["pend_fold_cms"], r["pend_fold_hll"], r["pend_fork"], r["pend_cap2"]) == (WHOLE, 1, 0, 0, 0), r
