// sa_server.hip — the HBM-streaming server kernels and their entries:
// sa_sum_u64 (masked-vector sum), sa_decode, sa_sum_f64 (weight sums).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/sfl_sa.h"
#include "sa_elems.h"
#include "sa_internal.h"

namespace sa {

// ---------------------------------------------------------------------------
// The server kernels stream HBM: 16-B accesses (two 8-B elements per lane and
// access), one tile of 256 x kUnroll accesses per block over a grid that
// covers the vector (no grid-stride loop), non-temporal loads and stores (the
// vectors are read once and written once).  tools/microbench/stream_rate.hip
// measured these choices on MI355X (profiles/r03/stream_rate.jsonl): copy
// 6.38 TB/s, two inputs 6.42, eight inputs 6.20, against 4.9-5.6 TB/s for an
// occupancy-sized grid-stride loop with default-policy accesses.  An odd last
// element is done by one lane of block 0.
// ---------------------------------------------------------------------------
constexpr int kUnroll = 4;
constexpr int kTileAccesses = 256 * kUnroll;  // 16-B accesses per block and input

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
using elems::f64x2;

template <typename T>
__device__ __forceinline__ T ld_nt(const T* p) {
  return __builtin_nontemporal_load(p);
}
template <typename T>
__device__ __forceinline__ void st_nt(T* p, T v) {
  __builtin_nontemporal_store(v, p);
}

// out = [out +] sum_k in[k], k <= kSumMaxIn, strictly left to right: the
// server sum (u64x2: mod 2^64) and the per-element weight sums (f64x2: the
// average's divisor vector); the documents and the profiles call the two
// k_sum_u64 and k_sum_f64.  V: the 16-B vector of two elements.  A chain of
// more inputs continues from `out` (accumulate).
template <typename V>
struct SumArgs {
  typedef decltype(V{}.x) T;
  const T* in[kSumMaxIn];
  T* out;
  uint64_t n;
  int k;
  int accumulate;
};

// inputs and out 16-B aligned
template <typename V>
__global__ void __launch_bounds__(256) k_sum(const SumArgs<V> a) {
  static_assert(sizeof(V) == 16 && sizeof(typename SumArgs<V>::T) == 8, "two 8-B elements per access");
  const uint64_t n2 = a.n / 2;
  const uint64_t base = (uint64_t)blockIdx.x * kTileAccesses + threadIdx.x;
  const int j0 = a.accumulate ? 0 : 1;
  const V* first = reinterpret_cast<const V*>(a.accumulate ? a.out : a.in[0]);
  V s[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; u++) s[u] = base + u * 256 < n2 ? ld_nt(first + base + u * 256) : V{0, 0};
  for (int j = j0; j < a.k; j++) {
    const V* in = reinterpret_cast<const V*>(a.in[j]);
#pragma unroll
    for (int u = 0; u < kUnroll; u++)
      if (base + u * 256 < n2) s[u] += ld_nt(in + base + u * 256);
  }
#pragma unroll
  for (int u = 0; u < kUnroll; u++)
    if (base + u * 256 < n2) st_nt(reinterpret_cast<V*>(a.out) + base + u * 256, s[u]);
  if ((a.n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    auto t = a.accumulate ? a.out[a.n - 1] : a.in[0][a.n - 1];
    for (int j = j0; j < a.k; j++) t += a.in[j][a.n - 1];
    a.out[a.n - 1] = t;
  }
}

// any alignment: one element per lane
__global__ void __launch_bounds__(256) k_sum_f64_unaligned(const SumArgs<f64x2> a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
    double s = a.accumulate ? a.out[i] : a.in[0][i];
    for (int j = a.accumulate ? 0 : 1; j < a.k; j++) s += a.in[j][i];
    a.out[i] = s;
  }
}

// decode: out = (double)(int64)s / 2^fxp / div
__device__ __forceinline__ double decode1(uint64_t s, double inv_scale, double div) {
  const double v = (double)(long long)s * inv_scale;  // exact power-of-two scaling
  return v / div;                                     // IEEE division
}

// s, out (and divv) 16-B aligned
template <bool kVec>
__global__ void __launch_bounds__(256) k_decode(const uint64_t* __restrict__ s, uint64_t n, double inv_scale,
                                                double div, const double* __restrict__ divv,
                                                double* __restrict__ out) {
  const uint64_t n2 = n / 2;
  const uint64_t base = (uint64_t)blockIdx.x * kTileAccesses + threadIdx.x;
  const u64x2* s2 = reinterpret_cast<const u64x2*>(s);
  const f64x2* d2 = reinterpret_cast<const f64x2*>(divv);
  f64x2* o2 = reinterpret_cast<f64x2*>(out);
  u64x2 v[kUnroll];
  f64x2 d[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; u++) {
    const bool in = base + u * 256 < n2;
    v[u] = in ? ld_nt(s2 + base + u * 256) : u64x2{0, 0};
    if (kVec) d[u] = in ? ld_nt(d2 + base + u * 256) : f64x2{1.0, 1.0};
  }
#pragma unroll
  for (int u = 0; u < kUnroll; u++)
    if (base + u * 256 < n2)
      st_nt(o2 + base + u * 256, f64x2{decode1(v[u].x, inv_scale, kVec ? d[u].x : div),
                                       decode1(v[u].y, inv_scale, kVec ? d[u].y : div)});
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    out[n - 1] = decode1(s[n - 1], inv_scale, kVec ? divv[n - 1] : div);
}

// any alignment (8-B elements one per lane): sub-vectors the caller sliced at odd offsets
__global__ void __launch_bounds__(256) k_decode_unaligned(const uint64_t* __restrict__ s, uint64_t n,
                                                          double inv_scale, double div,
                                                          const double* __restrict__ divv,
                                                          double* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    out[i] = decode1(s[i], inv_scale, divv ? divv[i] : div);
}

// one block per tile of kTileAccesses 16-B accesses (at least one block for
// the odd-element lane)
static int tile_grid(uint64_t n) {
  int grid;
  if (!tile_blocks((n / 2 + kUnroll - 1) / kUnroll, &grid)) {  // a lane's kUnroll accesses
    sa_set_error("vector of %llu elements exceeds one server-kernel launch", (unsigned long long)n);
    return -1;
  }
  return grid < 1 ? 1 : grid;
}

static int stream_grid(uint64_t work_items, const void* kfn) {
  const int maxb = occupancy_blocks(kfn);
  if (maxb <= 0) return -1;
  const uint64_t b = (work_items + 255) / 256;
  const uint64_t cap = (uint64_t)maxb;
  return (int)(b < 1 ? 1 : (b < cap ? b : cap));
}

// One launch of a server kernel chosen by its caller, over the grid of its
// kind for n elements: the 16-B kernels (tiled) take one block per tile, the
// any-alignment ones an occupancy-sized grid.
template <typename... A, typename... B>
static int launch_server(void (*fn)(A...), bool tiled, uint64_t n, void* stream, B... args) {
  const int grid = tiled ? tile_grid(n) : stream_grid(n, (const void*)fn);
  if (grid < 0) return tiled ? SA_ERR_ARG : SA_ERR_HIP;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(256), 0, (hipStream_t)stream, args...);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

// out = sum of in[0..k): launches of up to kSumMaxIn inputs, the later ones
// continuing from out
template <typename V, typename T>
static int launch_sum_chain(void (*fn)(const SumArgs<V>), bool tiled, const T* const* in, int k, uint64_t n, T* out,
                            void* stream) {
  for (int j0 = 0; j0 < k;) {
    SumArgs<V> a;
    memset(&a, 0, sizeof(a));
    a.accumulate = j0 > 0;
    while (a.k < kSumMaxIn && j0 < k) a.in[a.k++] = in[j0++];
    a.out = out;
    a.n = n;
    const int rc = launch_server(fn, tiled, n, stream, a);
    if (rc) return rc;
  }
  return SA_OK;
}

}  // namespace sa

using namespace sa;

extern "C" int sa_sum_u64(const uint64_t* const* in, int k, uint64_t n, uint64_t* out,
                          void* stream) {
  if (k >= 1 && n == 0) return SA_OK;  // empty vectors (their pointers may be null)
  if (!in || k < 1 || !out) {
    sa_set_error("sa_sum_u64: bad arguments (k=%d)", k);
    return SA_ERR_ARG;
  }
  for (int j = 0; j < k; j++)
    if (!in[j] || !aligned16(in[j])) {
      sa_set_error("sa_sum_u64: input %d null or not 16-byte aligned", j);
      return SA_ERR_ARG;
    }
  if (!aligned16(out)) {
    sa_set_error("sa_sum_u64: out not 16-byte aligned");
    return SA_ERR_ARG;
  }
  // out may alias in[0]: every lane reads its elements of in[0] before it writes them
  return launch_sum_chain(&k_sum<u64x2>, true, in, k, n, out, stream);
}

extern "C" int sa_decode(const uint64_t* s, uint64_t n, int fxp_bits, double divisor,
                         const double* divisor_vec, double* out, void* stream) {
  if (fxp_bits < 0 || fxp_bits > 62 || (n > 0 && (!s || !out))) {
    sa_set_error("sa_decode: bad arguments");
    return SA_ERR_ARG;
  }
  if (n == 0) return SA_OK;
  const double inv_scale = 1.0 / (double)((uint64_t)1 << fxp_bits);
  const bool vec = aligned16(s) && aligned16(out) && aligned16(divisor_vec);
  const auto fn = !vec ? &k_decode_unaligned : divisor_vec ? &k_decode<true> : &k_decode<false>;
  return launch_server(fn, vec, n, stream, s, n, inv_scale, divisor, divisor_vec, out);
}

extern "C" int sa_sum_f64(const double* const* w, int k, uint64_t n, double* out, void* stream) {
  if (k >= 1 && n == 0) return SA_OK;
  if (!w || k < 1 || !out) {
    sa_set_error("sa_sum_f64: bad arguments");
    return SA_ERR_ARG;
  }
  bool vec = aligned16(out);
  for (int j = 0; j < k; j++) {
    if (!w[j]) {
      sa_set_error("sa_sum_f64: input %d null", j);
      return SA_ERR_ARG;
    }
    vec = vec && aligned16(w[j]);
  }
  return launch_sum_chain(vec ? &k_sum<f64x2> : &k_sum_f64_unaligned, vec, w, k, n, out, stream);
}
