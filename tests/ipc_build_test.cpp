// Host-only print of the Hubble ipcache image as gpuagg_ipcache_set builds it (ipc_build,
// retina_amd/csrc/ipc_build.h): reads "sets", then per set "n" and n lines "ip identity meta"
// (decimal u32); prints per set one line "built cap max_probe" followed, for every input
// key in order, by "slot identity meta" of the slot that holds the key in the built image.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "ipc_build.h"

int main() {
  size_t sets = 0;
  if (scanf("%zu", &sets) != 1) return 2;
  for (size_t s = 0; s < sets; ++s) {
    size_t n = 0;
    if (scanf("%zu", &n) != 1) return 2;
    std::vector<uint32_t> ip(n), id(n), meta(n);
    for (size_t i = 0; i < n; ++i)
      if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &ip[i], &id[i], &meta[i]) != 3) return 2;
    gpuagg::IpcImage img;
    if (!gpuagg::ipc_build(ip.data(), id.data(), meta.data(), n, &img)) {
      printf("0 0 0\n");
      continue;
    }
    printf("1 %zu %" PRIu32, img.tab.size(), img.max_probe);
    for (size_t i = 0; i < n; ++i) {
      size_t at = img.tab.size();
      for (size_t k = 0; k < img.tab.size(); ++k)
        if (img.tab[k].ip == ip[i]) at = k;
      if (at == img.tab.size()) return 3;  // a key the image lost
      printf(" %zu %" PRIu32 " %" PRIu32, at, img.tab[at].identity, img.tab[at].meta);
    }
    printf("\n");
  }
  return 0;
}
