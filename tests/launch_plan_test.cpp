// Host-only check of the aggregation launch planner (retina_amd/csrc/gpuagg_launch_plan.h).
// One case per line of stdin, as "key=value" words: the facts of LaunchFacts / BatchFacts /
// PendingFacts by their field names (defaults below), the plan's groups as repeated
//   g=family:sparse:nsub:dense_base:key_mode:nbins
// and, for the edges no real plan reaches, force_lds_bins= / force_sig= replacing what
// plan_shape decided.  Prints one line per case: the plan's fields as "key=value" words, then
// name=<the variant's name> to the end of the line.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gpuagg_launch_plan.h"

using namespace gpuagg;

int main() {
  static char line[1 << 16];
  while (fgets(line, sizeof line, stdin)) {
    Plan p{};
    p.local = 1;
    LaunchFacts f{};
    f.plan = &p;
    f.seg_log2 = kSparseSegLog2;
    f.n_cu = 256;
    f.defer_folds = true;
    BatchFacts in{};
    in.aligned = 63;
    long long force_lds_bins = -1, force_sig = -1;
    bool any = false;
    for (char *tok = strtok(line, " \n"); tok; tok = strtok(nullptr, " \n")) {
      char *eq = strchr(tok, '=');
      if (!eq) return 2;
      *eq = 0;
      const char *key = tok, *val = eq + 1;
      any = true;
      if (!strcmp(key, "g")) {
        if (p.ngroups >= kMaxGroups) return 2;
        unsigned fam, sparse, nsub, km, nbins;
        unsigned long long base;
        if (sscanf(val, "%u:%u:%u:%llu:%u:%u", &fam, &sparse, &nsub, &base, &km, &nbins) != 6) return 2;
        GroupPlan &g = p.g[p.ngroups++];
        g.family = (uint8_t)fam, g.sparse = (uint8_t)sparse, g.nsub = nsub, g.dense_base = base, g.key_mode = km,
        g.nbins = nbins;
        continue;
      }
      const unsigned long long x = strtoull(val, nullptr, 10);
#define FACT(name, field) \
  if (!strcmp(key, name)) { field = (decltype(field))x; continue; }
      FACT("local", p.local)
      FACT("need_ports", p.need_ports)
      FACT("need_dns", p.need_dns)
      FACT("sparse_slots", f.sparse_slots)
      FACT("compact", f.compact)
      FACT("narrow", f.narrow)
      FACT("seg_log2", f.seg_log2)
      FACT("dense_len", f.dense_len)
      FACT("direct_sketch", f.direct_sketch)
      FACT("no_wide_lists", f.no_wide_lists)
      FACT("no_hot_keys", f.no_hot_keys)
      FACT("n_cu", f.n_cu)
      FACT("remote", f.remote)
      FACT("defer_folds", f.defer_folds)
      FACT("wide_list_bytes", f.wide_list_bytes)
      FACT("cms", f.cms)
      FACT("img_local.bytes", f.img_local.bytes)
      FACT("img_local.form", f.img_local.form)
      FACT("img_all.bytes", f.img_all.bytes)
      FACT("img_all.form", f.img_all.form)
      FACT("m", in.m)
      FACT("aligned", in.aligned)
      FACT("pend.active", in.pend.active)
      FACT("pend.nwin", in.pend.geom.nwin)
      FACT("pend.spill_cap", in.pend.geom.spill_cap)
      FACT("pend.win_blocks", in.pend.geom.win_blocks)
      FACT("pend.win_shift", in.pend.geom.win_shift)
      FACT("pend.sp_nwin", in.pend.geom.sp_nwin)
      FACT("pend.sp_cap", in.pend.geom.sp_cap)
      FACT("pend.budget", in.pend.budget)
      FACT("pend.rpb", in.pend.rpb)
      FACT("pend.blocks", in.pend.blocks)
      FACT("pend.lds_bins", in.pend.lds_bins)
      FACT("pend.dense_len", in.pend.dense_len)
      FACT("pend.same_state", in.pend.same_state)
      FACT("pend.staged", in.pend.staged)
      FACT("pend.stage_stride", in.pend.stage_stride)
      FACT("force_lds_bins", force_lds_bins)
      FACT("force_sig", force_sig)
#undef FACT
      fprintf(stderr, "unknown key %s\n", key);
      return 2;
    }
    if (!any) continue;
    LaunchShape s = plan_shape(f);
    if (force_lds_bins >= 0) s.lds_bins = (uint32_t)force_lds_bins;
    if (force_sig >= 0) s.sig = (uint32_t)force_sig;
    const BatchPlan b = plan_batch(f, s, in);
    const KernelVariant &v = b.variant;
    char name[64];
    variant_name(v, name, sizeof name);
    printf("dense_ng=%u dns_compact=%d tier1=%d lds_bins=%u sig=%u image=%d hot=%d sp_lists=%d shape_sp_nwin=%u "
           "stage_stride=%u blocks=%u threads=%u chunk=%llu hot_n=%u vec=%d nwin=%u spill_cap=%u win_blocks=%u "
           "win_shift=%u sp_nwin=%u sp_cap=%u budget=%llu defer=%d accum=%d stage_defer=%d stage_accum=%d "
           "fold_cond=%d row_masks=%d family=%d ng=%u v_vec=%d opt=%d excl=%d staged=%d kip=%d v_sig=%u "
           "lds_bytes=%u v_hot_n=%u door_log2=%u name=%s\n",
           s.dense_ng, (int)s.dns_compact, (int)s.tier1, s.lds_bins, s.sig, (int)s.image, (int)s.hot, (int)s.sp_lists,
           s.sp_nwin, s.stage_stride, s.blocks, s.threads, (unsigned long long)b.chunk, b.hot_n, (int)b.vec,
           b.geom.nwin, b.geom.spill_cap, b.geom.win_blocks, b.geom.win_shift, b.geom.sp_nwin, b.geom.sp_cap,
           (unsigned long long)b.budget, (int)b.defer, (int)b.accum, (int)b.stage_defer, (int)b.stage_accum,
           (int)b.fold_cond, (int)b.row_masks, (int)v.family, (unsigned)v.ng, (int)v.vec, (int)v.opt, (int)v.excl,
           (int)v.staged, (int)v.kip, v.sig, v.lds_bytes, v.hot_n, v.door_log2, name);
  }
  return 0;
}
