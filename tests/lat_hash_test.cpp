// Host-only print of the latency join's sort key (lat_hash, retina_amd/csrc/gpuagg_internal.h):
// reads "n" then n lines "k0 k1" (decimal u64) from stdin, prints one hash per line.
#include <cinttypes>
#include <cstdio>

#include "gpuagg_internal.h"

int main() {
  size_t n = 0;
  if (scanf("%zu", &n) != 1) return 2;
  for (size_t i = 0; i < n; ++i) {
    uint64_t k0 = 0, k1 = 0;
    if (scanf("%" SCNu64 " %" SCNu64, &k0, &k1) != 2) return 2;
    printf("%" PRIu64 "\n", gpuagg::lat_hash(k0, k1));
  }
  return 0;
}
