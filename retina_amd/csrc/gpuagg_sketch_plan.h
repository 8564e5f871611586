// The sketch launch planner: the count-min / HLL list geometry, the list capacities, the
// defer / accumulate policy, the scatter kernel and the fold shapes of a sketch pass, decided
// from plain facts.  Host-only (no HIP call, no ctx), so every rule here can be run and
// tested on a machine without a GPU (tests/sketch_plan_test.cpp).  launch_sketches,
// fold_pending_sketch and hh_fold_cms (gpuagg_runtime.cpp) gather the facts and act on the
// plan; launch_sketch (gpuagg_kernels.hip) dispatches on the variant, which
// sketch_variant_name() spells.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#include "gpuagg_internal.h"

namespace gpuagg {

// Count-min windows: 2^15 columns (128 KiB of LDS in the fold); at most 4096 windows
// (16 KiB of scatter counters), else every update is a direct global atomic.
constexpr uint32_t kCmsWindowShift = 15, kCmsMaxWindows = 4096;
// HLL windows: 2^shift source pods whose registers fit 128 KiB of LDS (entries carry the
// pod-in-window in 8 bits and the register index in 18, so p <= 17 and shift <= 8); more
// fine or super-windows than these: direct CAS.  (No row count reaches the super-window
// limit alone: past 1024 super-windows there are always more than 8192 fine ones.)
constexpr uint32_t kHllWindowLog2Bytes = 17, kHllMaxWindows = 8192, kHllMaxSuperWindows = 1024;

// Records per scatter workgroup between deferred sketch folds: 8 full-size C3 launches
// (2^27 records over 256 workgroups), 256 of the Go plugin's 2^22-record batches; ~15 GB of
// lists at C3's geometry (d = 4, 256 workgroups), plus the HLL re-bucketing lists at the
// fold.  Each fold rewrites the whole HLL register array and every count-min row, so fewer,
// larger folds pay that once per 8 launches instead of once per 2: C3 step 2.41 -> 2.30 ms
// (2^20 until round 6; 2^21: 2.37; profiles/round6/exp/r6k_c3_sketch_defer_budget_ab.jsonl).
constexpr uint64_t kSketchDeferRecords = 1ull << 22;

// sketch_stage_kernel holds a record's count-min updates in registers, unrolled over at
// most this many rows; deeper sketches take the unstaged kernel.
constexpr int kStageMaxDepth = 8;
// u32 words of sketch_stage_kernel's LDS before the IP image: rc, rb per window + hc, hb per
// super-window; u16 rings (+ one dummy u32); u32 rings (+ 64 dummies)
GA_HD uint32_t stage_words(uint32_t nwin, uint32_t hnsup, uint32_t sbc, uint32_t sbh) {
  return ((2u * (nwin + hnsup) + 3u) & ~3u) + ((nwin * sbc / 2u + 1u + 3u) & ~3u) + hnsup * sbh + 64u;
}

// ---- facts ---------------------------------------------------------------------------------
struct SketchFacts {
  uint32_t cms_depth, cms_wlog2;  // depth 0: no count-min
  uint32_t hll_p, hll_slots;      // p 0: no HLL; the rows its registers cover
  uint32_t n_cu;                  // scatter workgroups, one per CU
  bool direct_sketch;             // GPUAGG_FLAG_DIRECT_SKETCH
  bool defer_folds;
  LdsImageFacts img_all;          // the LDS image of every pod IP (source lookups)
};

// Per ctx: count-min windows of 2^win_shift columns (nwin 0: direct atomics), HLL fine
// windows of 2^hll_shift pods (128 KiB of registers, the fold's LDS) inside super-windows of
// 2^hll_sshift pods (~16 of them, the scatter's lists; hll_nsup 0: direct CAS), hll_b2 split
// workgroups per super-window.  Pod bits of an HLL entry: 26 - p.
struct SketchGeom {
  uint32_t win_shift = 0, nwin = 0, fold_blocks = 0;  // fold_blocks: a multiple of nwin
  uint32_t hll_shift = 0, hll_sshift = 0, hll_nwin = 0, hll_nsup = 0, hll_b2 = 0;
  bool operator==(const SketchGeom &o) const {
    return win_shift == o.win_shift && nwin == o.nwin && fold_blocks == o.fold_blocks && hll_shift == o.hll_shift &&
           hll_sshift == o.hll_sshift && hll_nwin == o.hll_nwin && hll_nsup == o.hll_nsup && hll_b2 == o.hll_b2;
  }
  uint32_t hll_nfine() const { return 1u << (hll_sshift - hll_shift); }  // fine windows per super-window
  size_t hll_lists2() const { return (size_t)hll_nsup * hll_b2 * hll_nfine(); }  // level-2 lists
};

inline SketchGeom sketch_geom(const SketchFacts &f) {
  SketchGeom g;
  g.win_shift = std::min(kCmsWindowShift, f.cms_wlog2);
  const uint64_t nwin = f.cms_depth ? (uint64_t)f.cms_depth << (f.cms_wlog2 - g.win_shift) : 0;
  if (!f.direct_sketch && nwin && nwin <= kCmsMaxWindows) {
    g.nwin = (uint32_t)nwin;
    g.fold_blocks = g.nwin * std::max(1u, f.n_cu / g.nwin);
  }
  if (!f.direct_sketch && f.hll_p && f.hll_p <= kHllWindowLog2Bytes && f.hll_slots) {
    g.hll_shift = std::min(8u, kHllWindowLog2Bytes - f.hll_p);
    auto windows = [&](uint32_t shift) { return ((uint64_t)f.hll_slots + (1u << shift) - 1) >> shift; };
    uint32_t ss = g.hll_shift;
    while (windows(ss) > 16 && ss < 26 - f.hll_p && ss < g.hll_shift + 10) ++ss;
    g.hll_sshift = ss;
    if (windows(g.hll_shift) <= kHllMaxWindows && windows(ss) <= kHllMaxSuperWindows) {
      g.hll_nwin = (uint32_t)windows(g.hll_shift);
      g.hll_nsup = (uint32_t)windows(ss);
    }
    g.hll_b2 = std::min(64u, std::max(1u, f.n_cu / std::max(1u, g.hll_nsup)));
  }
  return g;
}

// ---- list capacities -------------------------------------------------------------------------
// Entries of one list, for `rpb` records per scatter workgroup (one launch's chunk, or the
// deferral budget); a full list falls back to the exact global atomic / CAS.
// Count-min ([blocks][nwin] lists): rpb * depth / nwin expected, +12.5 % + 2048, whole 16 bytes.
inline uint32_t cms_list_cap(const SketchFacts &f, const SketchGeom &g, uint64_t rpb) {
  if (!g.nwin) return 0;
  const uint64_t mean = rpb * f.cms_depth / g.nwin;
  return (uint32_t)((mean + mean / 8 + 2048 + 7) & ~7ULL);
}
// HLL level 1 ([blocks][hll_nsup] lists): at most one entry per record, rpb / nsup per list,
// +25 % + 64, whole 64 bytes.
inline uint32_t hll_list_cap(const SketchGeom &g, uint64_t rpb) {
  if (!g.hll_nsup) return 0;
  const uint64_t mean = rpb / g.hll_nsup;
  return (uint32_t)((mean + mean / 4 + 64 + 15) & ~15ULL);
}
// HLL level 2 (the split's hll_lists2() lists) for `records` level-1 entries at most in all:
// the same headroom.
inline uint32_t hll_list2_cap(const SketchGeom &g, uint64_t records) {
  if (!g.hll_nsup) return 0;
  const uint64_t mean = records / g.hll_lists2();
  return (uint32_t)((mean + mean / 4 + 64 + 15) & ~15ULL);
}
struct SketchCaps {
  uint32_t cms = 0, hll = 0, hll2 = 0;
};

// ---- the scatter variant -----------------------------------------------------------------
struct SketchVariant {
  bool staged;  // sketch_stage_kernel<kip, kd>, else sketch_scatter_kernel<vec, lds_ip>
  uint8_t kip;  // source lookup: 0 HBM table, 1 LDS cuckoo image, 2 LDS radix image, 3 LDS dense radix image
  uint8_t kd;   // count-min depth fixed at compile time (4), or 0: the run-time loop
  bool vec;     // 16-byte loads
  bool lds_ip;  // the kernel is given the LDS image (staged: kip != 0)
  uint32_t round, sbc, sbh;  // staged: records per lane between flushes, ring entries per window / super-window
  uint32_t lds_bytes;        // dynamic LDS
};

// The kernel's signature as rocprofv3 prints it, without "void gpuagg::" and the argument list.
inline void sketch_variant_name(const SketchVariant &v, char *buf, size_t cap) {
  auto tf = [](bool b) { return b ? "true" : "false"; };
  if (v.staged) snprintf(buf, cap, "sketch_stage_kernel<%d, %d>", (int)v.kip, (int)v.kd);
  else snprintf(buf, cap, "sketch_scatter_kernel<%s, %s>", tf(v.vec), tf(v.lds_ip));
}

enum : uint32_t { kColSketchRead = kColSrcIp | kColDstIp | kColMeta | kColPorts };  // the columns the scatter loads

// The scatter kernel of a launch of `chunk` records per workgroup whose columns `aligned`
// (kCol*) start at a 16-byte boundary.
inline SketchVariant plan_sketch_variant(const SketchFacts &f, const SketchGeom &g, uint64_t chunk, uint32_t aligned) {
  SketchVariant v{};
  const uint32_t counters = ((g.nwin + g.hll_nsup + 3u) & ~3u) * 4;
  // source lookups in the LDS image of the IP table when it fits next to the plain counters
  const LdsImageFacts &img = f.img_all;
  const bool image = img.bytes && f.hll_p && (size_t)counters + img.bytes <= kLdsBytes;
  // 16-byte loads need aligned columns and workgroup chunks of whole vectors
  v.vec = chunk % 4 == 0 && (aligned & kColSketchRead) == kColSketchRead;
  // staged scatter: rings sized for a round's mean appends x 1.5 + 64 (the overflow goes
  // straight to the list), flushed every 4 records per lane, or every 2 when the 4-record
  // rings do not fit; either image form.  Depths above kStageMaxDepth take the unstaged
  // kernel (the staged one would stop at its unrolled rows and leave the rows above them at
  // zero), and so does any sketch that updates directly.
  if (v.vec && f.cms_depth <= (uint32_t)kStageMaxDepth && (!f.cms_depth || g.nwin) && (!f.hll_p || g.hll_nsup) &&
      (g.nwin || g.hll_nsup)) {
    auto ring = [](uint64_t mean) {
      uint32_t r = 64;
      while (r < mean + mean / 2 + 64) r <<= 1;
      return r;
    };
    for (uint32_t round : {4u, 2u}) {
      const uint64_t per_round = 1024ull * round;
      const uint32_t sbc = g.nwin ? ring(per_round * f.cms_depth / g.nwin) : 0u;
      const uint32_t sbh = g.hll_nsup ? ring(per_round / g.hll_nsup) : 0u;
      const size_t lds = (size_t)stage_words(g.nwin, g.hll_nsup, sbc, sbh) * 4 + (image ? img.bytes : 0u);
      if (lds > kLdsBytes) continue;
      v.staged = true;
      v.kip = image ? (uint8_t)(img.form + 1) : 0;
      v.kd = f.cms_depth == 4 ? 4 : 0;
      v.lds_ip = image;
      v.round = round;
      v.sbc = sbc;
      v.sbh = sbh;
      v.lds_bytes = (uint32_t)lds;
      return v;
    }
  }
  // the unstaged kernel probes the cuckoo image only: a radix image is looked up in HBM
  v.lds_ip = image && img.form == 0;
  v.lds_bytes = counters + (v.lds_ip ? img.bytes : 0u);
  return v;
}

// ---- the folds -----------------------------------------------------------------------------
struct SketchFoldShape {
  uint32_t cms_lds;         // cms_fold_kernel: one window of u32 counters
  uint32_t sbs, sbs_every;  // hll_split_kernel: ring entries per fine window (0: unstaged), rounds between flushes
  uint32_t split_lds;
  uint32_t hll_lds;         // hll_fold_kernel: a fine window's registers
};
inline SketchFoldShape plan_sketch_folds(uint32_t hll_p, const SketchGeom &g) {
  SketchFoldShape s{};
  if (g.nwin) s.cms_lds = 4u << g.win_shift;
  if (g.hll_nsup) {
    // staging rings: a round (4096 entries) over nfine windows, x 2 + 64, when they fit;
    // larger rings where LDS allows, flushed every few rounds (each flush is a barrier
    // pair for the workgroup): C3's 128 fine windows take 256-entry rings, every 3 rounds
    const uint32_t nfine = g.hll_nfine();
    const uint32_t per_round = 2 * 4096 / nfine;  // twice the mean appends per window
    uint32_t R = 64;
    while (R < per_round + 64) R <<= 1;
    if ((size_t)(2 + R) * nfine * 4 > kLdsBytes) R = 0;
    while (R && R < 256 && (size_t)(2 + 2 * R) * nfine * 4 <= kLdsBytes) R <<= 1;
    s.sbs = R;
    s.sbs_every = R ? std::max(1u, (R - 64) / std::max(1u, per_round)) : 1u;
    s.split_lds = (2 + R) * nfine * 4;
    s.hll_lds = 1u << (hll_p + g.hll_shift);
  }
  return s;
}

// ---- the plan of one launch_sketch call ------------------------------------------------------
struct SketchPlan {
  SketchGeom geom;
  SketchCaps caps;
  uint64_t chunk;  // records per scatter workgroup, whole 4-record vectors
  // which kernels run: the scatter, cms_fold, hll_split + hll_fold
  bool scatter, fold_cms, fold_hll;
  bool accum;  // the scatter appends after the fill earlier scatters stored (deferred folds)
  bool fork;   // both folds due: the count-min fold may run beside the HLL chain (disjoint state)
  SketchVariant variant;  // scatter
  SketchFoldShape fold;   // folds
};

// The folds of lists `caps` in geometry g (HLL precision hll_p); cms_only: the count-min fold
// alone (hh_fold_cms).
inline SketchPlan plan_sketch_fold(uint32_t hll_p, const SketchGeom &g, const SketchCaps &caps, bool cms_only = false) {
  SketchPlan p{};
  p.geom = g;
  p.caps = caps;
  p.fold_cms = g.nwin != 0;
  p.fold_hll = g.hll_nsup != 0 && !cms_only;
  p.fork = p.fold_cms && p.fold_hll;
  p.fold = plan_sketch_folds(hll_p, g);
  return p;
}
// A batch that scatters and folds runs as two launch_sketch calls, each timed on its own.
inline SketchPlan scatter_only(SketchPlan p) {
  p.fold_cms = p.fold_hll = p.fork = false;
  return p;
}
inline SketchPlan folds_only(SketchPlan p) {
  p.scatter = false;
  return p;
}

// ---- the submit ------------------------------------------------------------------------------
// The deferred scatters waiting for their folds (SketchPending).
struct SketchPendingFacts {
  bool active = false;
  SketchGeom geom;
  uint64_t rpb = 0, budget = 0;  // records per workgroup appended so far / the lists were sized for
  uint32_t blocks = 0;
  bool same_state = false;  // its rows, registers (and the rows they cover) and lists are still the ctx's
};
struct SketchSubmit {
  uint64_t per_launch;  // records of a batch: at most 2^20 per scatter workgroup
  // Deferred folds (small launches, e.g. the Go plugin's 2^20 records: chunk 4096): the
  // folds' fixed passes -- every count-min row and the whole HLL register array (164 MB at
  // C3's 10k pods, p = 14) are read and rewritten -- cost ~20x the scatter of such a launch,
  // so launches keep appending to one set of lists sized for `budget` records per workgroup
  // and fold_pending folds them once (gpuagg_sync, state reads, merge, relayout, or when the
  // next launch would not fit).
  bool defer;
  bool fold_first;  // the waiting set cannot take this submit: it is folded before
  bool accum;       // the submit appends to the waiting set's lists
  uint64_t budget;  // defer: records per workgroup the lists are sized for
};
inline uint64_t sketch_chunk(uint64_t m, uint32_t blocks) { return ((m + blocks - 1) / blocks + 3) & ~3ULL; }

inline SketchSubmit plan_sketch_submit(const SketchFacts &f, const SketchGeom &g, uint64_t n,
                                       const SketchPendingFacts &q) {
  SketchSubmit s{};
  s.per_launch = (uint64_t)f.n_cu << 20;
  const uint64_t chunk = sketch_chunk(std::min(n, s.per_launch), f.n_cu);
  // (2 * chunk <= kSketchDeferRecords cannot fail while a launch takes at most 2^20 records per
  // workgroup: 2^21 <= 2^22.  It guards a larger per_launch or a smaller budget and is the one
  // term no test reaches.  A count-min with more than kCmsMaxWindows windows still defers: its
  // updates are direct and the fold at the sync finds nothing to do.)
  s.defer = f.defer_folds && !f.direct_sketch && n <= s.per_launch && 2 * chunk <= kSketchDeferRecords &&
            (f.cms_depth || g.hll_nsup);
  s.accum = q.active && s.defer && q.rpb + chunk <= q.budget && q.blocks == f.n_cu && q.geom == g && q.same_state;
  s.fold_first = q.active && !s.accum;
  s.budget = s.accum ? q.budget : kSketchDeferRecords;
  return s;
}

// One batch of m records of the submit: a deferred batch only scatters (into lists sized for
// the budget); any other scatters into lists sized for itself and folds them at once.
inline SketchPlan plan_sketch_batch(const SketchFacts &f, const SketchGeom &g, const SketchSubmit &s, uint64_t m,
                                    uint32_t aligned) {
  SketchPlan p = plan_sketch_fold(f.hll_p, g, SketchCaps{});
  p.chunk = sketch_chunk(m, f.n_cu);
  const uint64_t rpb = s.defer ? s.budget : p.chunk;
  p.caps.cms = cms_list_cap(f, g, rpb);
  p.caps.hll = hll_list_cap(g, rpb);
  if (s.defer) p = scatter_only(p);
  else p.caps.hll2 = hll_list2_cap(g, m);
  p.scatter = true;
  p.accum = s.accum;
  p.variant = plan_sketch_variant(f, g, p.chunk, aligned);
  return p;
}

// hh_fold_cms: what of the waiting set the heavy-hitter test of a submit needs folded.
enum class HhFold : uint8_t {
  none,      // nothing waits, or the count-min updates were direct atomics
  cms_only,  // the count-min lists alone; the HLL lists stay deferred
  whole      // nothing of HLL waits: the ordinary fold of the waiting set
};
inline HhFold plan_hh_fold(const SketchPendingFacts &q) {
  if (!q.active || !q.geom.nwin) return HhFold::none;
  return q.geom.hll_nsup ? HhFold::cms_only : HhFold::whole;
}

}  // namespace gpuagg
