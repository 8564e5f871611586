// Host builder of the Hubble ipcache image that hubble_decode_kernel probes
// (gpuagg_hubble.hip; the CPU backend's Engine::hubble).  Header-only so that a host-only
// test (tests/ipc_build_test.cpp) exercises exactly the code gpuagg_ipcache_set runs.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "gpuagg_internal.h"

namespace gpuagg {

// The key of a free slot.  255.255.255.255 is therefore no ipcache key (ipc_build refuses
// it), and a probe for that address must miss: a free slot ends a probe before it can match.
constexpr uint32_t kIpcEmpty = 0xFFFFFFFFu;
constexpr uint32_t kIpcSeed = 0x7F4A7C15u;  // of ip_h1, fixed: the image is rebuilt whole

struct IpcEntry {  // the kernels read it as a uint4
  uint32_t ip, identity, meta, pad;
};
static_assert(sizeof(IpcEntry) == 16, "one 16-byte load per probe");

struct IpcImage {
  std::vector<IpcEntry> tab;  // 2^k slots, free ones {kIpcEmpty, 0, 0, 0}
  uint32_t max_probe = 0;     // the longest displacement of a key from its home slot
};

// Open addressing, linear probing from ip_h1(ip, kIpcSeed) & (cap - 1), load <= 50 %
// (64 slots, doubled while < 2n); the last entry for an IP wins.  Returns false, with
// *out untouched, when a key is kIpcEmpty.
inline bool ipc_build(const uint32_t *ipv4, const uint32_t *identity, const uint32_t *meta_id, size_t n,
                      IpcImage *out) {
  for (size_t i = 0; i < n; ++i)
    if (ipv4[i] == kIpcEmpty) return false;
  size_t cap = 64;
  while (cap < 2 * n) cap <<= 1;
  const uint32_t mask = (uint32_t)(cap - 1);
  out->tab.assign(cap, IpcEntry{kIpcEmpty, 0u, 0u, 0u});
  out->max_probe = 0;
  for (size_t i = 0; i < n; ++i) {
    uint32_t h = ip_h1(ipv4[i], kIpcSeed) & mask, p = 0;
    while (out->tab[h].ip != kIpcEmpty && out->tab[h].ip != ipv4[i]) {
      h = (h + 1) & mask;
      ++p;
    }
    out->tab[h] = IpcEntry{ipv4[i], identity[i], meta_id[i], 0u};
    if (p > out->max_probe) out->max_probe = p;
  }
  return true;
}

}  // namespace gpuagg
