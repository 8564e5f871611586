// The aggregation launch planner: which kernel a batch runs, and the LDS and list shapes it
// runs with, decided from plain facts.  Host-only (no HIP call, no ctx), so every rule here
// can be run and tested on a machine without a GPU (tests/launch_plan_test.cpp).
// launch() (gpuagg_runtime.cpp) gathers the facts and acts on the plan; launch_aggregate
// (gpuagg_kernels.hip) dispatches on the variant and names it with variant_name().
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <array>
#include <utility>

#include "gpuagg_internal.h"

namespace gpuagg {

// Launches whose list folds may wait for one fold_pending (see Pending).
constexpr uint64_t kDeferLaunches = 64;
// Spill-only plans defer their folds at launches of at most this many records per workgroup
// (the Go plugin's 2^22-record batches: 2^14; full-size launches fold per batch, see plan_batch).
constexpr uint64_t kSmallLaunchChunk = 1ull << 16;

// ---- the variant: one compiled kernel and its LDS ----------------------------------------
enum class KernelFamily : uint8_t { aggregate, wide, dense_local, dense_lds };
struct KernelVariant {
  KernelFamily family;
  // template arguments, in each family's order (the others 0 / false / -1)
  uint8_t ng;     // wide_kernel 2 / 4; dense kernels 1 / 2 / 4 / 8
  bool vec;       // every column 16-byte aligned: dwordx4 loads
  bool opt;       // dense_local: dns; aggregate: sketch; wide: remote
  bool excl;      // wide: no two groups of one family
  bool staged;    // dense_local: spill appends staged in LDS rings
  int8_t kip;     // form of the LDS IP image: 0 cuckoo, 1 row radix, 2 dense radix; wide: -1 none
  uint32_t sig;   // SIG of a compile-time specialised signature, else 0
  uint32_t lds_bytes;  // dynamic LDS
  uint32_t hot_n;      // LDS hot-key cache entries, a power of two (0: none)
  uint32_t door_log2;  // log2 bits of the hot-key cache's doorkeeper bitmap (0: none)
};

// The kernel's signature as rocprofv3 prints it, without "void gpuagg::" and the argument list.
inline void variant_name(const KernelVariant &v, char *buf, size_t cap) {
  auto tf = [](bool b) { return b ? "true" : "false"; };
  switch (v.family) {
    case KernelFamily::wide:
      snprintf(buf, cap, "wide_kernel<%d, %s, %s, %d>", (int)v.ng, tf(v.opt), tf(v.excl), (int)v.kip);
      break;
    case KernelFamily::dense_lds:
      snprintf(buf, cap, "dense_lds_kernel<%u, %s, %uu, %d>", (unsigned)v.ng, tf(v.vec), v.sig, (int)v.kip);
      break;
    case KernelFamily::dense_local:
      snprintf(buf, cap, "dense_local_kernel<%u, %s, %s, %uu%s>", (unsigned)v.ng, tf(v.vec), tf(v.opt), v.sig,
               v.staged ? ", true" : "");
      break;
    case KernelFamily::aggregate:
      snprintf(buf, cap, "aggregate_kernel<%s, %s>", tf(v.vec), tf(v.opt));
      break;
  }
}

// ---- facts ---------------------------------------------------------------------------------
struct LaunchFacts {
  const Plan *plan;
  uint64_t sparse_slots;  // group-by table (0: none)
  bool compact, narrow;   // SparseView
  uint32_t seg_log2;
  uint64_t dense_len;
  bool direct_sketch, no_wide_lists, no_hot_keys;  // GPUAGG_FLAG_*
  uint32_t n_cu;
  bool remote, defer_folds;
  uint64_t wide_list_bytes;
  bool cms;                  // count-min on: it reads the ports column
  LdsImageFacts img_local;   // tier-1: the local pods
  LdsImageFacts img_all;     // every pod
};

// List geometry: spill lists per fold window for the bins past the LDS window, compact- or
// wide-key lists per table segment.
struct ListGeom {
  uint32_t nwin = 0, spill_cap = 0, win_blocks = 0, sp_nwin = 0, sp_cap = 0, win_shift = 0;
  bool operator==(const ListGeom &o) const {
    return nwin == o.nwin && spill_cap == o.spill_cap && win_blocks == o.win_blocks && sp_nwin == o.sp_nwin &&
           sp_cap == o.sp_cap && win_shift == o.win_shift;
  }
};

// The deferred launches waiting for their fold (Pending).
struct PendingFacts {
  bool active = false;
  ListGeom geom;
  uint64_t budget = 0, rpb = 0;
  uint32_t blocks = 0, lds_bins = 0;
  uint64_t dense_len = 0;
  bool same_state = false;  // its counters and table are still the ctx's
  bool staged = false;      // it keeps tier-1 copies (stage_defer) in the buffer this launch would use
  uint32_t stage_stride = 0;
};
struct BatchFacts {
  uint64_t m;        // records
  uint32_t aligned;  // kCol* of the columns that start at a 16-byte boundary (a null column does)
  PendingFacts pend;
};

// ---- the plan ------------------------------------------------------------------------------
enum class LdsImage : uint8_t { none, local, all };
struct LaunchShape {  // the same for every batch of one launch() call
  uint32_t dense_ng;  // 0: generic kernel; 1/2/4/8: dense local-context kernel
  bool dns_compact;   // dense kernel also inserts the compact plan's DNS keys (segment lists)
  bool tier1;         // dense kernel with the IP table and u32 bins in LDS
  uint32_t lds_bins;  // dense bins [0, lds_bins) privatised in LDS
  uint32_t sig;       // group signature (kSig*), 0 when the plan has none
  LdsImage image;     // the LDS IP image the kernel is given
  bool hot;           // LDS hot-key cache in front of the group-by table
  bool sp_lists;      // group-by keys bucketed per table segment
  uint32_t sp_nwin;   // their number, one per table segment (0: none)
  uint32_t stage_stride;  // tier-1: words per workgroup copy of the LDS bins, summed after (0: no copies)
  uint32_t blocks, threads;
};
struct BatchPlan {
  uint64_t chunk;  // records per workgroup, multiple of 4
  uint32_t hot_n;  // hot-key cache entries before the variant re-sizes them
  bool vec;
  ListGeom geom;
  uint64_t budget;        // records per workgroup the lists are sized for
  bool defer;             // the list folds wait for fold_pending
  bool accum;             // the lists hold the pending launches' entries
  bool stage_defer, stage_accum, fold_cond;  // LaunchArgs
  bool row_masks;         // spilled tcpflags rows 8-aligned in their windows: one row-mask entry
  KernelVariant variant;
};

namespace plan_detail {
struct DenseSpans {  // (base, bins) of the dense groups, sorted
  std::array<std::pair<uint64_t, uint64_t>, kMaxGroups> s;
  int n = 0;
  explicit DenseSpans(const Plan &p) {
    for (int g = 0; g < p.ngroups; ++g)
      if (!p.g[g].sparse) s[n++] = {p.g[g].dense_base, p.g[g].nbins};
    std::sort(s.begin(), s.begin() + n);
  }
  // LDS window: the longest prefix of whole dense groups (hottest first) that fits
  uint32_t prefix(uint64_t limit) const {
    uint32_t L = 0;
    for (int i = 0; i < n; ++i) {
      if (s[i].first != L || s[i].first + s[i].second > limit) break;
      L = (uint32_t)(s[i].first + s[i].second);
    }
    return L;
  }
};
// groups in layout order, as the kernel indexes them
inline uint32_t signature(const Plan &p, uint32_t lds_bins) {
  uint32_t sig = 0;
  if (p.ngroups > 8) return 0;
  for (int g = 0; g < p.ngroups; ++g)
    sig |= sig_group(p.g[g].family, !p.g[g].sparse && p.g[g].dense_base + p.g[g].nbins <= lds_bins) << (4 * g);
  return sig;
}
// the largest doorkeeper bitmap (2^13 .. 2^18 bits) that fits behind `lds` bytes; 0: none
inline uint32_t door_fit(size_t lds) {
  for (uint32_t l = 18; l >= 13; --l)
    if (lds + ((size_t)1 << (l - 3)) <= kLdsBytes) return l;
  return 0;
}
}  // namespace plan_detail

// geometry: one 1024-thread workgroup per CU holding L dense bins in LDS
inline LaunchShape plan_shape(const LaunchFacts &f) {
  const Plan &p = *f.plan;
  LaunchShape s{};
  // dense local-context fast path: every group dense (sketches run in their own pass,
  // launch_sketches, so the metric groups keep the dense fast paths)
  if (p.local && p.ngroups > 0) {
    // every group dense, or -- compact plan -- dense and DNS (keys of 64 bits, inserted
    // through the segment lists by the dense kernel)
    bool all_dense = true;
    for (int g = 0; g < p.ngroups; ++g) {
      const bool dns = p.g[g].family == FAM_DNS_REQ || p.g[g].family == FAM_DNS_RESP;
      if (p.g[g].sparse && f.compact && dns && f.sparse_slots &&
          (f.sparse_slots >> f.seg_log2) <= kSparseMaxSegLists && !f.direct_sketch)
        s.dns_compact = true;
      else
        all_dense &= !p.g[g].sparse;
    }
    if (!all_dense) s.dns_compact = false;
    if (all_dense)
      for (uint32_t ng : {1u, 2u, 4u, 8u})
        if ((uint32_t)p.ngroups <= ng) {
          s.dense_ng = ng;
          break;
        }
  }
  const plan_detail::DenseSpans spans(p);
  // compact group-by keys (generic kernel) go through per-segment lists whose fill
  // counters take LDS words from the dense window
  const bool generic = !s.dense_ng || s.dns_compact;  // kernels that take compact-key lists
  const uint64_t sp_nwin = f.sparse_slots ? f.sparse_slots >> f.seg_log2 : 0;
  // wide (192-bit) keys take per-segment lists too when the table has at most 4096
  // segments of 2^12 slots (sparse_fold_wide_kernel folds one per workgroup)
  const bool wide_lists = !f.compact && f.sparse_slots && f.sparse_slots <= (1ull << kWideMaxLog2) && !f.no_wide_lists;
  s.sp_lists = generic && (f.compact || wide_lists) && sp_nwin && sp_nwin <= kSparseMaxSegLists && !f.direct_sketch;
  s.sp_nwin = s.sp_lists ? (uint32_t)sp_nwin : 0u;
  // plans with HBM-table keys (remote context, ip / port options): an LDS cache of the
  // hot keys per workgroup in front of the table (hot_add in gpuagg_kernels.hip)
  s.hot = generic && f.sparse_slots && !f.compact && !f.no_hot_keys;
  s.lds_bins = spans.prefix(kLdsMaxBins - (s.sp_nwin + 1) / 2 - (s.hot ? kHotKeys * kHotKeyBytes / 8 + 1 : 0u));
  if (s.dense_ng && s.dns_compact) s.sig = plan_detail::signature(p, s.lds_bins);  // dense_local_kernel's signature
  // tier-1: the LDS IP image plus u32 bins, when at least the image fits
  // (with no group in LDS every update spills, but the IP probes still stay on-chip)
  if (s.dense_ng && !s.dns_compact && f.img_local.bytes && f.img_local.bytes + kL4ExtraBytes < kLdsBytes) {
    s.tier1 = true;
    s.lds_bins = spans.prefix((kLdsBytes - f.img_local.bytes - kL4ExtraBytes) / 4);
    s.sig = plan_detail::signature(p, s.lds_bins);
    s.image = LdsImage::local;
    if (s.lds_bins) s.stage_stride = (s.lds_bins + 3u) & ~3u;
  }
  // remote context on the wide-key path: the LDS image of every pod IP (wide_kernel takes
  // it when it fits next to the hot-key cache; the context never reads the apiserver flag)
  if (s.hot && f.remote && !s.tier1 && f.img_all.bytes) s.image = LdsImage::all;
  // one 1024-thread workgroup per CU whenever LDS holds bins or spill counters: with
  // dense bins but no LDS prefix (C5: 100k-pod groups) 4x fewer workgroups mean 4x
  // fewer, longer spill lists for the fold (same 16 waves per CU)
  // (the hot-key cache alone fills ~2/3 of the LDS: with 256-thread workgroups a CU would
  // run 4 waves)
  const bool big = s.lds_bins || s.tier1 || f.dense_len > 0 || s.hot;
  s.blocks = big ? f.n_cu : f.n_cu * 4;
  s.threads = big ? 1024 : 256;
  return s;
}

// u64 words of a segment-list entry: a compact key, or a wide key's 32 (narrow: 24) bytes
inline uint32_t list_entry_words(bool compact, bool narrow) {
  return compact ? 1u : narrow ? kWideNarrowWords : kWideEntryWords;
}

// List geometry for `budget` records per workgroup: spill lists per fold window for
// the bins past the LDS window (overflow falls back to global atomics; a multiple of 4
// keeps lists 16-byte aligned), compact-key lists per table segment (at most one
// insert per record, hashed evenly: budget / nwin per list + 25 % + 64; a full list
// inserts in place, exact).
inline ListGeom list_geom(const LaunchFacts &f, const LaunchShape &s, uint64_t budget) {
  ListGeom g;
  if (f.dense_len > s.lds_bins) {
    const uint64_t rem = f.dense_len - s.lds_bins;
    const uint32_t shift = kFoldWindowShift;
    const uint32_t nwin = (uint32_t)((rem + (1ull << shift) - 1) >> shift);
    const uint64_t cap = ((2 * budget / nwin + 4096) + 3) & ~3ULL;
    if (nwin <= kMaxSpillWindows && cap < (1u << 24)) {  // 24-bit index math in the kernels
      g.nwin = nwin;
      g.win_shift = shift;
      g.spill_cap = (uint32_t)cap;
      g.win_blocks = nwin * std::max<uint32_t>(1u, 2u * f.n_cu / nwin);  // one wave of 2 per CU
    }
  }
  if (s.sp_lists) {
    const uint64_t mean = budget / s.sp_nwin;
    g.sp_nwin = s.sp_nwin;
    uint64_t cap = (mean + mean / 4 + 64 + 1) & ~1ULL;  // even: 16-byte key pairs
    if (!f.compact)  // wide_list_bytes of lists per ctx
      cap = std::max<uint64_t>(16, f.wide_list_bytes / (8 * list_entry_words(false, f.narrow)) /
                                       ((uint64_t)s.blocks * s.sp_nwin)) & ~1ULL;
    g.sp_cap = (uint32_t)cap;
  }
  return g;
}

// The kernel of a batch, its dynamic LDS, and the hot-key cache and doorkeeper that fit in it.
inline KernelVariant plan_variant(const LaunchFacts &f, const LaunchShape &s, const BatchPlan &b) {
  const Plan &p = *f.plan;
  const LdsImageFacts img = s.image == LdsImage::local ? f.img_local : s.image == LdsImage::all ? f.img_all : LdsImageFacts{0, 0};
  KernelVariant v{};
  v.vec = b.vec;
  v.kip = -1;
  v.hot_n = b.hot_n;
  const uint32_t sp_nwin = b.geom.sp_nwin;
  size_t lds = s.tier1 ? (size_t)img.bytes + (size_t)s.lds_bins * 4 + kL4ExtraBytes
                       : ((size_t)s.lds_bins + kLdsExtraWords) * 8 + (size_t)sp_nwin * 4 +
                             (b.hot_n ? 4 + (size_t)b.hot_n * kHotKeyBytes : 0);
  // the hot-key cache's doorkeeper bitmap takes what LDS is left (2^13 .. 2^18 bits) on the
  // wide-key list path, where any key may otherwise claim an entry
  const bool wide_path = !s.tier1 && b.hot_n && sp_nwin && !f.compact;
  // sparse-only plans on the wide-key list path (no dense group, no tcpflags, <= 4 groups):
  // wide_kernel
  bool wide = wide_path && !s.dense_ng && b.vec && p.ngroups >= 1 && p.ngroups <= 4;
  bool excl = true;
  for (int g = 0; wide && g < p.ngroups; ++g) {
    wide = p.g[g].sparse && p.g[g].family != FAM_TCPFLAGS;
    for (int h = 0; h < g; ++h) excl &= p.g[h].family != p.g[g].family;
  }
  if (wide) {
    v.family = KernelFamily::wide;
    v.ng = p.ngroups > 2 ? 4 : 2;
    v.opt = !p.local;
    v.excl = excl;
    // LDS: (remote context) the image of every pod IP when it fits next to a cache of
    // >= kWideIplMinHot entries and a 2^kWideIplMinDoor-bit doorkeeper (the cache halves
    // until it does), counters, cache, then the largest doorkeeper bitmap that fits
    const size_t ctr = (size_t)((sp_nwin + 1) / 2) * 8;
    const size_t ib = v.opt && s.image != LdsImage::none ? ((size_t)img.bytes + 15) & ~15ull : 0;
    const size_t min_door = (size_t)1 << (kWideIplMinDoor - 3);
    if (ib) {
      uint32_t hn = v.hot_n;
      while (hn > kWideIplMinHot && ib + ctr + (size_t)hn * kHotKeyBytes + min_door > kLdsBytes) hn >>= 1;
      if (ib + ctr + (size_t)hn * kHotKeyBytes + min_door <= kLdsBytes) {
        v.kip = img.form;
        v.hot_n = hn;
      }
    }
    lds = (v.kip >= 0 ? ib : 0) + ctr + (size_t)v.hot_n * kHotKeyBytes;
  }
  if (wide_path) v.door_log2 = plan_detail::door_fit(lds);
  if (v.door_log2) lds += (size_t)1 << (v.door_log2 - 3);
  if (s.tier1) {
    v.family = KernelFamily::dense_lds;
    v.kip = img.form;
    // compile-time specialised signatures: the common C2 shapes
    const bool special = s.sig == kSigFwdLdsDropSpill || s.sig == kSigFwdLdsDropLds || s.sig == kSigFwdLds;
    v.sig = special ? s.sig : 0u;
    v.ng = (uint8_t)(!special ? s.dense_ng : s.sig == kSigFwdLds ? 1u : 2u);
  } else if (s.dense_ng) {
    v.family = KernelFamily::dense_local;
    v.ng = (uint8_t)s.dense_ng;
    v.opt = s.dns_compact;  // with the compact plan's DNS groups (segment lists)
    if (s.dns_compact && s.dense_ng == 4 && s.sig == kSigC5) {
      v.sig = kSigC5;
      const size_t rings = (size_t)b.geom.nwin * (1 + kSpillRing) * 4;
      if (b.geom.nwin && lds + rings <= kLdsBytes) {  // spill appends staged in LDS rings
        v.staged = true;
        lds += rings;
      }
    }
  } else if (!wide) {
    v.family = KernelFamily::aggregate;  // (sketches run in their own pass: never <., true>)
  }
  v.lds_bytes = (uint32_t)lds;
  return v;
}

inline BatchPlan plan_batch(const LaunchFacts &f, const LaunchShape &s, const BatchFacts &in) {
  const Plan &p = *f.plan;
  const PendingFacts &q = in.pend;
  BatchPlan b{};
  b.chunk = ((in.m + s.blocks - 1) / s.blocks + 3) & ~3ULL;
  if (s.hot) {
    // the cache is flushed into the lists once per workgroup and launch: at small batches
    // (the Go plugin's 1M records: 4k per workgroup) a full 2048-entry cache doubled the
    // appends, so it is sized ~chunk / 8 (256 .. kHotKeys entries; under Zipf(1.2) the
    // top 256 keys still carry ~70 % of the updates)
    uint32_t hn = 256;
    while (hn < kHotKeys && (uint64_t)hn * 16 <= b.chunk) hn <<= 1;
    b.hot_n = hn;
  }
  const uint32_t read = kColSrcIp | kColDstIp | kColBytes | kColMeta | (p.need_ports || f.cms ? kColPorts : 0u) |
                        (p.need_dns ? kColDnsId : 0u);
  b.vec = (in.aligned & read) == read;
  // Deferred folds: while the geometry holds, launches keep appending to the same lists
  // (their counters start from the stored fill) for up to kDeferLaunches (64) launches' worth
  // of records per workgroup, and fold_pending folds them once.
  // Plans with compact-key lists always defer: their fold pays a fixed pass over the
  // group-by table.  Spill-only plans (C2, C4) defer only small launches (at most
  // kMaxRecordsPerBlock / kDeferLaunches records per workgroup, e.g. the Go plugin's 2^20
  // records): there the spill fold's fixed pass over the windows cost more than the
  // tier-1 kernel itself; at full-size launches appending past earlier launches' entries
  // measured ~2 % slower in the tier-1 kernel (profiles/round2/r4f_*), so they fold per batch.
  const bool small_spill = f.dense_len > s.lds_bins && b.chunk <= kSmallLaunchChunk;
  const bool defer = f.defer_folds && (s.sp_lists || small_spill);
  // Wide lists (192-bit keys) are folded when the device says so: every launch's fold
  // skips itself until some list is half full (sparse_fold_wide_kernel), so the host keeps
  // appending without a record budget -- under skew the LDS hot-key cache absorbs most
  // updates and a budget that assumes one entry per record folded ~5x too often.
  b.fold_cond = defer && s.sp_lists && !f.compact;
  b.budget = defer ? std::max<uint64_t>(b.chunk, std::min<uint64_t>(kMaxRecordsPerBlock, kDeferLaunches * b.chunk))
                   : b.chunk;
  if (b.fold_cond) b.budget = ~0ull >> 1;
  b.accum = q.active && defer && q.rpb + b.chunk <= q.budget && list_geom(f, s, q.budget) == q.geom &&
            q.blocks == s.blocks && q.lds_bins == s.lds_bins && q.dense_len == f.dense_len && q.same_state;
  if (b.accum) b.budget = q.budget;
  b.geom = list_geom(f, s, b.budget);
  b.defer = defer && (b.geom.nwin || b.geom.sp_nwin);
  // small spill-only launches keep the tier-1 copies too: each workgroup continues from
  // its staged copy and the copies are summed once, by the deferred fold -- the per-launch
  // stage_reduce_kernel (reading blocks x the LDS bins) was most of such a launch's cost
  b.stage_defer = b.defer && small_spill && !s.sp_lists && s.stage_stride;
  b.stage_accum = b.stage_defer && b.accum && q.staged && q.stage_stride == s.stage_stride;
  // row-mask spill entries need every tcpflags group's 8-bin rows aligned in the windows
  b.row_masks = b.geom.nwin != 0;
  for (int g = 0; g < p.ngroups; ++g)
    if (p.g[g].family == FAM_TCPFLAGS && !p.g[g].sparse &&
        (p.g[g].nsub != 8 || p.g[g].dense_base < s.lds_bins || (p.g[g].dense_base - s.lds_bins) % 8))
      b.row_masks = false;
  b.variant = plan_variant(f, s, b);
  return b;
}

}  // namespace gpuagg
