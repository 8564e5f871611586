// Host-only check of the sketch launch planner (retina_amd/csrc/gpuagg_sketch_plan.h).
// One case per line of stdin, as "key=value" words: the facts of SketchFacts and
// SketchPendingFacts by their field names (defaults below), n= the records of the submit and
// aligned= the batch's column mask.  Prints one line per case: the geometry, the submit's plan,
// its first batch's plan (and the record count, chunk and folds of its last batch), the fold of
// the waiting set as fold_pending_sketch and hh_fold_cms would plan it, as "key=value" words, then
// name=<the scatter variant's name> to the end of the line.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gpuagg_sketch_plan.h"

using namespace gpuagg;

int main() {
  static char line[1 << 12];
  while (fgets(line, sizeof line, stdin)) {
    SketchFacts f{};
    f.n_cu = 256;
    f.defer_folds = true;
    SketchPendingFacts q;
    unsigned long long n = 0;
    uint32_t aligned = 63;
    bool any = false;
    for (char *tok = strtok(line, " \n"); tok; tok = strtok(nullptr, " \n")) {
      char *eq = strchr(tok, '=');
      if (!eq) return 2;
      *eq = 0;
      const char *key = tok;
      const unsigned long long x = strtoull(eq + 1, nullptr, 10);
      any = true;
#define FACT(name, field) \
  if (!strcmp(key, name)) { field = (decltype(field))x; continue; }
      FACT("cms_depth", f.cms_depth)
      FACT("cms_wlog2", f.cms_wlog2)
      FACT("hll_p", f.hll_p)
      FACT("hll_slots", f.hll_slots)
      FACT("n_cu", f.n_cu)
      FACT("direct_sketch", f.direct_sketch)
      FACT("defer_folds", f.defer_folds)
      FACT("img_all.bytes", f.img_all.bytes)
      FACT("img_all.form", f.img_all.form)
      FACT("n", n)
      FACT("aligned", aligned)
      FACT("pend.active", q.active)
      FACT("pend.win_shift", q.geom.win_shift)
      FACT("pend.nwin", q.geom.nwin)
      FACT("pend.fold_blocks", q.geom.fold_blocks)
      FACT("pend.hll_shift", q.geom.hll_shift)
      FACT("pend.hll_sshift", q.geom.hll_sshift)
      FACT("pend.hll_nwin", q.geom.hll_nwin)
      FACT("pend.hll_nsup", q.geom.hll_nsup)
      FACT("pend.hll_b2", q.geom.hll_b2)
      FACT("pend.rpb", q.rpb)
      FACT("pend.budget", q.budget)
      FACT("pend.blocks", q.blocks)
      FACT("pend.same_state", q.same_state)
#undef FACT
      fprintf(stderr, "unknown key %s\n", key);
      return 2;
    }
    if (!any) continue;
    const SketchGeom g = sketch_geom(f);
    const SketchSubmit s = plan_sketch_submit(f, g, n, q);
    // the batches as launch_sketches walks them
    unsigned batches = 0;
    unsigned long long last_m = 0;
    SketchPlan first{}, last{};
    for (unsigned long long off = 0; off < n; off += s.per_launch) {
      last_m = n - off < s.per_launch ? n - off : s.per_launch;
      last = plan_sketch_batch(f, g, s, last_m, aligned);
      if (!batches++) first = last;
    }
    const SketchPlan &b = first;
    const SketchVariant &v = b.variant;
    // the waiting set's folds
    SketchCaps qc;
    qc.hll2 = hll_list2_cap(q.geom, q.rpb * q.blocks);
    const SketchPlan pf = plan_sketch_fold(f.hll_p, q.geom, qc);
    const HhFold hh = plan_hh_fold(q);
    const SketchPlan ph = plan_sketch_fold(f.hll_p, q.geom, qc, true);
    char name[64];
    sketch_variant_name(v, name, sizeof name);
    printf("win_shift=%u nwin=%u fold_blocks=%u hll_shift=%u hll_sshift=%u hll_nwin=%u hll_nsup=%u hll_b2=%u "
           "per_launch=%llu defer=%d fold_first=%d accum=%d budget=%llu batches=%u last_m=%llu last_chunk=%llu "
           "last_fold_cms=%d last_fold_hll=%d chunk=%llu cap=%u hll_cap=%u hll_cap2=%u scatter=%d fold_cms=%d "
           "fold_hll=%d b_accum=%d fork=%d staged=%d kip=%d kd=%d vec=%d lds_ip=%d round=%u sbc=%u sbh=%u lds_bytes=%u "
           "cms_lds=%u sbs=%u sbs_every=%u split_lds=%u hll_lds=%u "
           "pend_fold_cms=%d pend_fold_hll=%d pend_fork=%d pend_cap2=%u hh=%d hh_fold_cms=%d hh_fold_hll=%d hh_fork=%d "
           "name=%s\n",
           g.win_shift, g.nwin, g.fold_blocks, g.hll_shift, g.hll_sshift, g.hll_nwin, g.hll_nsup, g.hll_b2,
           (unsigned long long)s.per_launch, (int)s.defer, (int)s.fold_first, (int)s.accum, (unsigned long long)s.budget,
           batches, last_m, (unsigned long long)last.chunk, (int)last.fold_cms, (int)last.fold_hll,
           (unsigned long long)b.chunk, b.caps.cms, b.caps.hll, b.caps.hll2, (int)b.scatter, (int)b.fold_cms,
           (int)b.fold_hll, (int)b.accum, (int)b.fork, (int)v.staged, (int)v.kip, (int)v.kd, (int)v.vec, (int)v.lds_ip,
           v.round, v.sbc, v.sbh, v.lds_bytes, b.fold.cms_lds, b.fold.sbs, b.fold.sbs_every, b.fold.split_lds,
           b.fold.hll_lds, (int)pf.fold_cms, (int)pf.fold_hll, (int)pf.fork, pf.caps.hll2, (int)hh, (int)ph.fold_cms,
           (int)ph.fold_hll, (int)ph.fork, name);
  }
  return 0;
}
