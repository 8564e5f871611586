// Sketch readouts on gfx950: which flows are the heavy hitters (count-min) and how many
// distinct peers every pod has (HyperLogLog), without moving the sketches to the host.
//
//  * hh_candidate_kernel streams a submit's records once more, after its count-min updates
//    are in the rows, and hands every key whose estimate has reached min_count to the
//    candidate table: a set of exact 128-bit keys in HBM that persists across submits.
//  * hh_count_kernel / hh_export_kernel / hh_rank_kernel / hh_select_kernel /
//    hh_gather_kernel read that table: the number of candidates, their keys, and the k
//    largest by their current estimate (rocprim radix sort on (estimate, slot)).
//  * hll_estimate_kernel reduces every pod's registers to three exact integers, from which
//    the host applies gpuagg_hll_estimate's estimator.
//
// The candidate table: 2^L slots of a 16-byte key (src_ip, dst_ip, ports, proto) and a tag
// word, open addressing with linear probing from the key's home slot, nothing ever removed.
// Tag: 0 free; kHhPending | h while the claimer writes the key; kHhFull | h once it is
// there (h = 29 bits of the key's hash, so a probe reads the key of a slot only when the
// hash bits agree and waits at a pending slot only when it may be its own key); kHhDup
// marks the later of two slots that hold one key.  Two slots can come to hold one key only
// when a lane gives up its bounded wait at a pending slot; hh_count_kernel, which every
// read runs first, finds such a slot by probing from its home, so a key is counted,
// exported and ranked once.  Every word of the table is written and read with agent-scope
// atomics inside hh_candidate_kernel (workgroups on different XCDs share it); the read
// kernels run in later launches and use plain loads.
#include <hip/hip_runtime.h>

#include <cstring>  // rocprim's texture iterator uses memset

#include <rocprim/rocprim.hpp>

#include "gpuagg_internal.h"
#include "gpuagg_launch.h"

namespace gpuagg {

namespace {

constexpr uint32_t kHhFull = 0x80000000u, kHhPending = 0x40000000u, kHhDup = 0x20000000u, kHhHash = (1u << kHhTagBits) - 1u;
static_assert((kHhDup & kHhHash) == 0 && kHhDup == kHhHash + 1u, "the tag word: three state bits above the hash bits");
// re-reads of a pending slot that may hold this key before probing on (the kFoldSpin
// convention of the group-by folds: the claimer publishes within a few instructions, the
// bound keeps every insert finite); the pass path is rare, so the bound is generous
constexpr uint32_t kHhSpin = 256;
// per-workgroup LDS set of the keys this workgroup has handed on: 2^11 entries of 20 bytes,
// kHhLdsProbe slots tried (a key that finds none of them free is simply not remembered)
constexpr uint32_t kHhLds = 1u << kHhLdsLog2, kHhLdsProbe = 4;

struct HhK {
  const uint32_t *src, *dst, *ports, *meta;
  uint64_t n, chunk;
  const uint32_t *cms;
  uint32_t depth, wlog2, min_count;
  uint4 *keys;
  uint32_t *tags;
  uint32_t mask;
  unsigned long long *words;
};

// (hh_home, hh_hash, hh_lds_home: gpuagg_launch.h)
__device__ __forceinline__ bool key_eq(const uint4 &a, const uint4 &b) {
  return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
}

// The count-min estimate of one key: the minimum of its column in each of d rows.
__device__ __forceinline__ uint32_t cms_min(const uint32_t *cms, uint32_t depth, uint32_t wlog2, uint64_t base) {
  const uint32_t wmask = (1u << wlog2) - 1u;
  uint32_t m = 0xFFFFFFFFu;
  for (uint32_t r = 0; r < depth; ++r) m = min(m, cms[((size_t)r << wlog2) + cms_col(base, r, wmask)]);
  return m;
}

__device__ __forceinline__ uint32_t tag_load(const uint32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint4 key_load(const uint4 *p) {  // of a slot whose tag reads full
  const uint32_t *w = (const uint32_t *)p;
  return make_uint4(tag_load(w), tag_load(w + 1), tag_load(w + 2), tag_load(w + 3));
}

// Insert-if-absent of one key by a whole converged wave (every lane holds the same key):
// the loads are the wave's, the claim, the key's stores and the counters lane 0's.  Bounded:
// at most mask + 1 probes and kHhSpin re-reads.  A full table counts the key in
// words[kHhWordDropped].
__device__ __forceinline__ void hh_insert(const HhK &k, const uint4 &key, uint64_t base) {
  const uint32_t h = hh_hash(base), home = hh_home(base, k.mask);
  const bool first = (threadIdx.x & 63u) == 0;
  uint32_t spin = 0;
  for (uint32_t probe = 0; probe <= k.mask;) {
    const uint32_t i = (home + probe) & k.mask;
    uint32_t t = tag_load(&k.tags[i]);
    if (t == 0u) {
      uint32_t prev = 0u;
      if (first) prev = atomicCAS(&k.tags[i], 0u, kHhPending | h);
      prev = __shfl(prev, 0);
      if (prev == 0u) {
        if (first) {
          uint32_t *w = (uint32_t *)&k.keys[i];
          __hip_atomic_store(w, key.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(w + 1, key.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(w + 2, key.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(w + 3, key.w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(&k.tags[i], kHhFull | h, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);  // publish
        }
        return;
      }
      t = prev;  // claimed this instant by another wave
    }
    if (t & kHhFull) {
      if ((t & kHhHash) == h) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (key_eq(key_load(&k.keys[i]), key)) return;  // already a candidate
      }
      ++probe;
      continue;
    }
    // pending: another key's slot unless the hash bits agree; then wait for it (bounded)
    // rather than taking a second slot
    if ((t & kHhHash) == h && spin < kHhSpin) {
      ++spin;
      __builtin_amdgcn_s_sleep(2);
      continue;
    }
    ++probe;
  }
  if (first) atomicAdd(&k.words[kHhWordDropped], 1ULL);
}

struct HhLds {
  uint32_t *tag;
  uint4 *key;
};
// (a converged wave, one key) true: this workgroup has handed the key on already
__device__ __forceinline__ bool hh_lds_find(const HhLds &L, const uint4 &key, uint64_t base) {
  const uint32_t want = kHhFull | hh_hash(base), i0 = hh_lds_home(base);
  for (uint32_t q = 0; q < kHhLdsProbe; ++q) {
    const uint32_t i = (i0 + q) & (kHhLds - 1u);
    const uint32_t t = __hip_atomic_load(&L.tag[i], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (t == 0u) return false;  // entries fill in probe order and never leave
    if (t == want && key_eq(L.key[i], key)) return true;
  }
  return false;
}
__device__ __forceinline__ void hh_lds_insert(const HhLds &L, const uint4 &key, uint64_t base) {
  const uint32_t i0 = hh_lds_home(base);
  const bool first = (threadIdx.x & 63u) == 0;
  for (uint32_t q = 0; q < kHhLdsProbe; ++q) {
    const uint32_t i = (i0 + q) & (kHhLds - 1u);
    uint32_t prev = 1u;
    if (first) prev = atomicCAS(&L.tag[i], 0u, kHhPending);
    prev = __shfl(prev, 0);
    if (prev != 0u) continue;
    if (first) {
      L.key[i] = key;
      __hip_atomic_store(&L.tag[i], kHhFull | hh_hash(base), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    return;
  }
}

// One record per lane of a converged wave, `pass` where its estimate has reached min_count:
// the wave takes the passing lanes' distinct keys one at a time (a key many lanes hold --
// the heavy flow itself -- is one turn), each first looked up in the LDS set, then handed
// to the table and remembered.  At most 64 turns.
__device__ __forceinline__ void hh_wave_pass(const HhK &k, const HhLds &L, bool pass, const uint4 &key, uint64_t base) {
  unsigned long long m = __ballot(pass);
  while (m) {
    const int leader = __ffsll((long long)m) - 1;
    const uint4 lk = make_uint4(__shfl(key.x, leader), __shfl(key.y, leader), __shfl(key.z, leader),
                                __shfl(key.w, leader));
    const uint64_t lb = (uint64_t)__shfl((uint32_t)base, leader) | ((uint64_t)__shfl((uint32_t)(base >> 32), leader) << 32);
    m &= ~__ballot(pass && key_eq(key, lk));
    if (hh_lds_find(L, lk, lb)) continue;
    hh_insert(k, lk, lb);
    hh_lds_insert(L, lk, lb);
  }
}

// The candidate pass over one submit's records: sketch_stage_kernel's streaming skeleton
// (one 1024-thread workgroup per CU over a contiguous chunk, kVec: 4 records per lane per
// step from 16-byte loads, the next step's loads in flight), per record cms_base once, d
// gathers from the rows (L2 / Infinity Cache resident), their minimum against min_count.
// Every loop has a block-uniform trip count, so the waves reach hh_wave_pass converged.
template <bool kVec>
__global__ __launch_bounds__(1024) void hh_candidate_kernel(HhK k) {
  __shared__ __attribute__((aligned(16))) uint4 lkey[kHhLds];
  __shared__ uint32_t ltag[kHhLds];
  for (uint32_t i = threadIdx.x; i < kHhLds; i += blockDim.x) ltag[i] = 0u;
  __syncthreads();
  const HhLds L{ltag, lkey};
  const uint64_t start = (uint64_t)blockIdx.x * k.chunk;
  if (start >= k.n) return;  // block-uniform: a chunk that starts past the records
  const uint64_t end = start + k.chunk < k.n ? start + k.chunk : k.n;
  const uint32_t wmask = (1u << k.wlog2) - 1u, T = k.min_count;
  uint64_t tail = start;
  if (kVec && start + 4 <= end) {
    const uint64_t v0 = start >> 2, vend = v0 + ((end - start) >> 2);
    const uint4 *s4 = (const uint4 *)k.src, *d4 = (const uint4 *)k.dst;
    const uint4 *p4 = (const uint4 *)k.ports, *m4 = (const uint4 *)k.meta;
    const uint4 z4 = make_uint4(0, 0, 0, 0);
    uint4 ns = z4, nd = z4, nm = z4, np = z4;
    if (v0 + threadIdx.x < vend) {
      const uint64_t v = v0 + threadIdx.x;
      ns = s4[v];
      nd = d4[v];
      nm = m4[v];
      np = p4 ? p4[v] : z4;
    }
    for (uint64_t vb = v0; vb < vend; vb += blockDim.x) {
      const uint64_t v = vb + threadIdx.x;
      const bool a = v < vend;
      const uint4 vs = ns, vd = nd, vm = nm, vp = np;
      const uint64_t vn = v + blockDim.x;
      if (vn < vend) {
        ns = s4[vn];
        nd = d4[vn];
        nm = m4[vn];
        np = p4 ? p4[vn] : z4;
      }
      const uint4 key[4] = {make_uint4(vs.x, vd.x, vp.x, meta_proto(vm.x)), make_uint4(vs.y, vd.y, vp.y, meta_proto(vm.y)),
                            make_uint4(vs.z, vd.z, vp.z, meta_proto(vm.z)), make_uint4(vs.w, vd.w, vp.w, meta_proto(vm.w))};
      uint64_t base[4];
      uint32_t est[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        base[j] = cms_base(key[j].x, key[j].y, key[j].z, key[j].w);
        est[j] = 0xFFFFFFFFu;
      }
      // the four records' gathers of a row issued together
      for (uint32_t r = 0; r < k.depth; ++r) {
        const uint32_t *row = k.cms + ((size_t)r << k.wlog2);
        uint32_t c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = row[cms_col(base[j], r, wmask)];
#pragma unroll
        for (int j = 0; j < 4; ++j) est[j] = min(est[j], c[j]);
      }
      bool pass[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) pass[j] = a && est[j] >= T;
      if (__builtin_expect(__ballot(pass[0] | pass[1] | pass[2] | pass[3]) != 0, 0)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) hh_wave_pass(k, L, pass[j], key[j], base[j]);
      }
    }
    tail = start + ((end - start) & ~3ULL);
  }
  // scalar loads: columns off a 16-byte boundary, and the ragged tail of the last chunk
  for (uint64_t ib = tail; ib < end; ib += blockDim.x) {
    const uint64_t i = ib + threadIdx.x;
    const bool a = i < end;
    const uint4 key = a ? make_uint4(k.src[i], k.dst[i], k.ports ? k.ports[i] : 0u, meta_proto(k.meta[i])) : make_uint4(0, 0, 0, 0);
    const uint64_t base = cms_base(key.x, key.y, key.z, key.w);
    const bool pass = a && cms_min(k.cms, k.depth, k.wlog2, base) >= T;
    if (__ballot(pass) != 0) hh_wave_pass(k, L, pass, key, base);
  }
}

// Host keys (gpuagg_hh_add_candidates, the merge): one wave per key.
__global__ __launch_bounds__(256) void hh_add_kernel(HhK k, const uint4 *in, size_t n) {
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((size_t)gridDim.x * blockDim.x) >> 6;
  for (size_t i = wave; i < n; i += nwaves) {
    const uint4 key = in[i];
    hh_insert(k, key, cms_base(key.x, key.y, key.z, key.w));
  }
}

// Marks the later slots of a key that holds two (probing from the key's home to the slot:
// every slot on the way is occupied, nothing is ever removed) and counts the others into
// words[kHhWordCount], one add per wave.
__global__ __launch_bounds__(256) void hh_count_kernel(HhK k) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool live = false;
  if (i <= k.mask) {
    const uint32_t t = k.tags[i];
    live = (t & kHhFull) && !(t & kHhDup);
    if (live) {
      const uint4 key = k.keys[i];
      for (uint32_t j = hh_home(cms_base(key.x, key.y, key.z, key.w), k.mask); j != (uint32_t)i; j = (j + 1) & k.mask) {
        const uint32_t tj = k.tags[j];
        if ((tj & kHhFull) && (tj & kHhHash) == (t & kHhHash) && key_eq(k.keys[j], key)) {
          __hip_atomic_fetch_or(&k.tags[i], kHhDup, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          live = false;
          break;
        }
      }
    }
  }
  const unsigned long long b = __ballot(live);
  if ((threadIdx.x & 63u) == 0 && b) atomicAdd(&k.words[kHhWordCount], (unsigned long long)__popcll(b));
}

// (after hh_count_kernel) every candidate key behind words[kHhWordCursor], in any order
__global__ __launch_bounds__(256) void hh_export_kernel(HhK k, uint4 *out, size_t cap) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > k.mask) return;
  const uint32_t t = k.tags[i];
  if (!(t & kHhFull) || (t & kHhDup)) return;
  const unsigned long long pos = atomicAdd(&k.words[kHhWordCursor], 1ULL);
  if (pos < cap) out[pos] = k.keys[i];
}

// (after hh_count_kernel) one sort key per slot: (2^32 - 1 - estimate) << 32 | slot for a
// candidate, all ones for a free or duplicate slot -- ascending order is estimate descending
__global__ __launch_bounds__(256) void hh_rank_kernel(HhK k, unsigned long long *sort_in) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > k.mask) return;
  const uint32_t t = k.tags[i];
  unsigned long long v = ~0ULL;
  if ((t & kHhFull) && !(t & kHhDup)) {
    const uint4 key = k.keys[i];
    const uint32_t est = cms_min(k.cms, k.depth, k.wlog2, cms_base(key.x, key.y, key.z, key.w));
    v = ((unsigned long long)(0xFFFFFFFFu - est) << 32) | (unsigned long long)i;
  }
  sort_in[i] = v;
}

// The sorted keys' prefix to hand over: the kk largest and every further candidate whose
// estimate ties the kk-th (the host finishes the order among equal estimates).  One
// thread finds the end of that run.  kk >= 1 and at most the number of candidates.
__global__ __launch_bounds__(256) void hh_select_kernel(const unsigned long long *sorted, size_t slots, size_t kk,
                                                         unsigned long long *words) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= slots || i + 1 < kk) return;
  const uint32_t hk = (uint32_t)(sorted[kk - 1] >> 32);
  const bool in = sorted[i] != ~0ULL && (uint32_t)(sorted[i] >> 32) == hk;
  const bool next = i + 1 < slots && sorted[i + 1] != ~0ULL && (uint32_t)(sorted[i + 1] >> 32) == hk;
  if (in && !next) words[kHhWordSelect] = (unsigned long long)(i + 1);
}

__global__ __launch_bounds__(256) void hh_gather_kernel(HhK k, const unsigned long long *sorted, size_t m, HhEntry *out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const unsigned long long s = sorted[i];
  const uint4 key = k.keys[(uint32_t)s & k.mask];
  out[i] = HhEntry{key.x, key.y, key.z, key.w, (uint64_t)(0xFFFFFFFFu - (uint32_t)(s >> 32))};
}

// Distinct peers: one pod's 2^p registers reduced to three exact integers -- the registers
// that are zero, sum 2^(32 - r) over r <= 32 and sum 2^(64 - r) over r > 32 (ranks are at
// most 65 - p and m <= 2^18, so neither sum passes 2^50 and the order does not matter).
// kWave: a wave per pod (p <= 12: at most four 16-byte loads per lane), else a workgroup.
__device__ __forceinline__ void hll_acc(uint32_t word, uint32_t &zeros, unsigned long long &lo, unsigned long long &hi) {
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const uint32_t r = (word >> (8 * b)) & 0xFFu;
    zeros += r == 0u;
    if (r <= 32u) lo += 1ULL << (32u - r);
    else if (r <= 64u) hi += 1ULL << (64u - r);
  }
}
template <bool kWave>
__global__ __launch_bounds__(256) void hll_estimate_kernel(const uint8_t *hll, uint32_t p, uint32_t rows,
                                                            unsigned long long *out) {
  __shared__ unsigned long long part[3][4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t pod = kWave ? blockIdx.x * 4u + wave : blockIdx.x;
  const uint32_t t = kWave ? lane : threadIdx.x, stride = kWave ? 64u : 256u;
  uint32_t zeros = 0;
  unsigned long long lo = 0, hi = 0;
  if (pod < rows) {
    const uint8_t *reg = hll + ((size_t)pod << p);
    const uint32_t m = 1u << p;
    if (m >= 16u) {
      const uint4 *r4 = (const uint4 *)reg;
      for (uint32_t i = t; i < (m >> 4); i += stride) {
        const uint4 v = r4[i];
        hll_acc(v.x, zeros, lo, hi);
        hll_acc(v.y, zeros, lo, hi);
        hll_acc(v.z, zeros, lo, hi);
        hll_acc(v.w, zeros, lo, hi);
      }
    } else if (t == 0) {  // p < 4: a few bytes
      for (uint32_t i = 0; i < m; ++i) {
        const uint32_t r = reg[i];
        zeros += r == 0u;
        if (r <= 32u) lo += 1ULL << (32u - r);
        else if (r <= 64u) hi += 1ULL << (64u - r);
      }
    }
  }
  unsigned long long z = zeros;
  for (int off = 32; off > 0; off >>= 1) {
    z += __shfl_down(z, off);
    lo += __shfl_down(lo, off);
    hi += __shfl_down(hi, off);
  }
  if (kWave) {
    if (lane == 0 && pod < rows) {
      out[3 * (size_t)pod] = z;
      out[3 * (size_t)pod + 1] = lo;
      out[3 * (size_t)pod + 2] = hi;
    }
    return;
  }
  if (lane == 0) {
    part[0][wave] = z;
    part[1][wave] = lo;
    part[2][wave] = hi;
  }
  __syncthreads();
  if (threadIdx.x < 3 && pod < rows)
    out[3 * (size_t)pod + threadIdx.x] = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
}

HhK hh_k(const HhTable &t) {
  HhK k{};
  k.cms = t.cms;
  k.depth = t.cms_depth;
  k.wlog2 = t.cms_wlog2;
  k.keys = t.keys;
  k.tags = t.tags;
  k.mask = t.mask;
  k.words = (unsigned long long *)t.words;
  return k;
}
dim3 per_slot(const HhTable &t) { return dim3((uint32_t)(((size_t)t.mask + 1 + 255) / 256)); }

}  // namespace

hipError_t launch_hh_candidates(const HhArgs &a, hipStream_t st) {
  if (!a.n) return hipSuccess;
  HhK k = hh_k(a.table);
  k.src = a.cols.src_ip;
  k.dst = a.cols.dst_ip;
  k.ports = a.cols.ports;
  k.meta = a.cols.meta;
  k.n = a.n;
  k.chunk = a.chunk;
  k.min_count = a.min_count;
  // 16-byte loads need aligned columns and workgroup chunks of whole vectors
  const bool vec = a.chunk % 4 == 0 && ((uintptr_t)k.src | (uintptr_t)k.dst | (uintptr_t)k.meta |
                                        (uintptr_t)(k.ports ? k.ports : k.src)) % 16 == 0;
  if (vec) hipLaunchKernelGGL(hh_candidate_kernel<true>, dim3(a.blocks), dim3(1024), 0, st, k);
  else hipLaunchKernelGGL(hh_candidate_kernel<false>, dim3(a.blocks), dim3(1024), 0, st, k);
  return hipGetLastError();
}

hipError_t launch_hh_add(const HhTable &t, const uint32_t *keys4, size_t n, hipStream_t st) {
  if (!n) return hipSuccess;
  const uint32_t blocks = (uint32_t)std::min<size_t>((n + 3) / 4, 4096);
  hipLaunchKernelGGL(hh_add_kernel, dim3(blocks), dim3(256), 0, st, hh_k(t), (const uint4 *)keys4, n);
  return hipGetLastError();
}

hipError_t launch_hh_count(const HhTable &t, hipStream_t st) {
  hipError_t e = hipMemsetAsync(t.words + kHhWordCount, 0, 8, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(hh_count_kernel, per_slot(t), dim3(256), 0, st, hh_k(t));
  return hipGetLastError();
}

hipError_t launch_hh_export(const HhTable &t, uint32_t *out4, size_t cap, hipStream_t st) {
  hipError_t e = hipMemsetAsync(t.words + kHhWordCursor, 0, 8, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(hh_export_kernel, per_slot(t), dim3(256), 0, st, hh_k(t), (uint4 *)out4, cap);
  return hipGetLastError();
}

hipError_t hh_sort_bytes(size_t slots, size_t *bytes) {
  return rocprim::radix_sort_keys(nullptr, *bytes, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                  slots, 0, 64, (hipStream_t)0);
}

hipError_t launch_hh_rank(const HhTable &t, uint64_t *sort_in, uint64_t *sort_out, void *tmp, size_t tmp_bytes,
                          size_t kk, hipStream_t st) {
  const size_t slots = (size_t)t.mask + 1;
  hipLaunchKernelGGL(hh_rank_kernel, per_slot(t), dim3(256), 0, st, hh_k(t), (unsigned long long *)sort_in);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  size_t tb = tmp_bytes;
  if ((e = rocprim::radix_sort_keys(tmp, tb, (const unsigned long long *)sort_in, (unsigned long long *)sort_out, slots,
                                    0, 64, st)) != hipSuccess)
    return e;
  if ((e = hipMemsetAsync(t.words + kHhWordSelect, 0, 8, st)) != hipSuccess) return e;
  hipLaunchKernelGGL(hh_select_kernel, per_slot(t), dim3(256), 0, st, (const unsigned long long *)sort_out, slots, kk,
                     (unsigned long long *)t.words);
  return hipGetLastError();
}

hipError_t launch_hh_gather(const HhTable &t, const uint64_t *sorted, size_t m, HhEntry *out, hipStream_t st) {
  if (!m) return hipSuccess;
  hipLaunchKernelGGL(hh_gather_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, st, hh_k(t),
                     (const unsigned long long *)sorted, m, out);
  return hipGetLastError();
}

hipError_t launch_hll_estimate(const uint8_t *hll, uint32_t p, uint32_t rows, uint64_t *out3, hipStream_t st) {
  if (!rows) return hipSuccess;
  if (p <= 12) hipLaunchKernelGGL(hll_estimate_kernel<true>, dim3((rows + 3) / 4), dim3(256), 0, st, hll, p, rows,
                                  (unsigned long long *)out3);
  else hipLaunchKernelGGL(hll_estimate_kernel<false>, dim3(rows), dim3(256), 0, st, hll, p, rows,
                          (unsigned long long *)out3);
  return hipGetLastError();
}

}  // namespace gpuagg
