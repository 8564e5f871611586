// Host-only check of the group-by key hashes (retina_amd/csrc/gpuagg_internal.h).  One key per
// line of stdin as three decimal u64 words "k0 k1 k2"; prints, per key, key_hash(k0, k1, k2) and
// fmix64(k0 ^ 0x243F6A8885A308D3) -- the compact table's hash of the 64-bit key k0 (compact_home
// before the mask, gpuagg_kernels.hip) -- in decimal.
#include <cinttypes>
#include <cstdio>

#include "gpuagg_internal.h"

int main() {
  unsigned long long k0, k1, k2;
  while (scanf("%llu %llu %llu", &k0, &k1, &k2) == 3)
    printf("%" PRIu64 " %" PRIu64 "\n", (uint64_t)gpuagg::key_hash(k0, k1, k2),
           (uint64_t)gpuagg::fmix64(k0 ^ 0x243F6A8885A308D3ULL));
  return 0;
}
