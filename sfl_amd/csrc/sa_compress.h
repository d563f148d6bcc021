// sa_compress.h — what the compression translation units share (sa_stc.hip,
// sa_scr.hip, sa_coo.hip, sa_topk.hip, and through sa_runs.h sa_quant.hip and
// sa_kmeans.hip; sa_flame.hip, the robust aggregator's passes, takes the wave
// layout and the entry checks too; nothing else includes it; sa_stc.hip and sa_topk.hip add
// sa_select.h, the radix select): the block
// shape, the contiguous wave layout with its launch geometry and the block
// scan on the device; the element-type dispatch and the first checks of an
// entry on the host.  A new compressor starts from here.  (The wave sums stay
// loops in their kernels: behind a function the compiler schedules them
// differently.)
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sfl_sa.h"
#include "sa_elems.h"
#include "sa_internal.h"

namespace sa {
namespace wave {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

// --- the contiguous wave layout -------------------------------------------
// Every wave owns one index range of `len` elements (a multiple of kTile),
// waves in index order, so wave order is index order.
constexpr int kTileBlock = elems::kTile * kWaves;
constexpr int kMaxBlocks = 1024;  // 4 resident blocks per CU on 256 CUs
constexpr int kMaxWaves = kMaxBlocks * kWaves;

// this wave's index range [lo, hi)
struct Range {
  uint64_t lo, hi;
  int lane;
};
__device__ __forceinline__ Range wave_range(uint64_t n, uint64_t len) {
  const uint64_t w = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  Range r;
  r.lo = w * len < n ? w * len : n;
  r.hi = r.lo + len < n ? r.lo + len : n;
  r.lane = threadIdx.x & 63;
  return r;
}

// The launch of n elements in this layout.  A function of n only, so the
// passes over one tensor agree on every wave's range and a float64 sum has
// one order; `ptrs`: the vectors' addresses OR-ed (16-byte accesses if all
// are 16-byte aligned).  At least one block, also for n == 0.
struct Grid {
  int grid, nwaves, vec;
  uint64_t len;
};
inline Grid wave_grid(uint64_t n, uintptr_t ptrs) {
  uint64_t blocks = (n + kTileBlock - 1) / kTileBlock;
  if (blocks > (uint64_t)kMaxBlocks) blocks = kMaxBlocks;
  if (blocks == 0) blocks = 1;
  Grid g;
  g.grid = (int)blocks, g.nwaves = g.grid * kWaves;
  g.len = (n + g.nwaves - 1) / g.nwaves;
  g.len = (g.len + elems::kTile - 1) / elems::kTile * elems::kTile;
  g.vec = (ptrs & 15) == 0;
  return g;
}

// inclusive scan of one value per thread over the block (thread order)
__device__ __forceinline__ uint32_t block_scan_incl(uint32_t s, uint32_t* total) {
  __shared__ uint32_t wsum[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = s;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t v = (uint32_t)__shfl_up((int)inc, off, 64);
    if (lane >= off) inc += v;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t base = 0, all = 0;
  for (int i = 0; i < kWaves; i++) {
    if (i < wave) base += wsum[i];
    all += wsum[i];
  }
  *total = all;
  return base + inc;
}

}  // namespace wave

// --- an entry's first steps (host) ------------------------------------------
namespace entry {

inline uintptr_t elem_size(int t) { return t == SA_F32 ? 4 : 8; }
inline bool misaligned(const void* p, uintptr_t esz) { return ((uintptr_t)p & (esz - 1)) != 0; }

// SA_OK, or SA_ERR_ARG with "<what>: <noun> must be SA_F32 or SA_F64" set
inline int check_float(int t, const char* what, const char* noun = "the element type") {
  if (t != SA_F32 && t != SA_F64) {
    sa_set_error("%s: %s must be SA_F32 or SA_F64", what, noun);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

// SA_OK, or SA_ERR_ARG with "<what>: n must be below 2^<bits><why>" set
inline int check_n(uint64_t n, int bits, const char* what, const char* why = "") {
  if (n >> bits) {
    sa_set_error("%s: n must be below 2^%d%s", what, bits, why);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

// the element type, then the size: what most entries check first
inline int check_float_n(int t, uint64_t n, int bits, const char* what, const char* why = "") {
  const int rc = check_float(t, what);
  return rc != SA_OK ? rc : check_n(n, bits, what, why);
}

// f(T()) with T the element type of x_type (checked before): float or double
template <class F>
inline auto dispatch_float(int x_type, F&& f) {
  if (x_type == SA_F32) return f(float());
  return f(double());
}

}  // namespace entry
}  // namespace sa
