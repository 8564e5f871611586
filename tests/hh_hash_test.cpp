// Host-only check of the hash slices the heavy-hitter readout takes from a key's count-min base
// (retina_amd/csrc/gpuagg_internal.h, gpuagg_launch.h).  One key per line of stdin as four decimal
// u32 words "src_ip dst_ip ports proto"; prints, per key, cms_base and of it hh_home under a
// full mask (base >> kHhHomeShift, 32 bits: a table's home is its low capacity_log2 bits),
// hh_hash (the tag) and hh_lds_home -- in decimal.
#include <cinttypes>
#include <cstdio>

#include "gpuagg_launch.h"

int main() {
  unsigned a, b, c, d;
  while (scanf("%u %u %u %u", &a, &b, &c, &d) == 4) {
    const uint64_t base = gpuagg::cms_base(a, b, c, d);
    printf("%" PRIu64 " %u %u %u\n", base, gpuagg::hh_home(base, 0xFFFFFFFFu), gpuagg::hh_hash(base),
           gpuagg::hh_lds_home(base));
  }
  return 0;
}
