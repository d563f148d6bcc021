// sa_flame.hip — the per-element work of FlameAggregator on the device (the
// reference's robust aggregator, examples/security/h_bd/agg_flame.py:27-203;
// sfl_amd/security/aggregation/flame_aggregator.py has the definition and the
// host form, DESIGN.md §19 the passes and the resource table):
//
//   stats   = one pass (two for more than kFusedClients clients) over the C
//             clients' tensors: the element-wise median g, every client's
//             sum of (x_i - g)^2 and the Gram matrix sum of x_i x_j, in
//             float64, as per-block partials; then one block that joins the
//             partials in block order
//   combine = one streaming pass: g and the kept clients in, the clipped
//             weighted average out, float64
//
// Both run on sa_compress.h's contiguous wave layout, so the grid and every
// wave's range are functions of n only and a float64 sum has one order: a
// lane's tiles in index order, the lanes of a wave by a fixed butterfly, the
// waves of a block in wave order, the blocks in block order.  No atomics.
// The C values of an element are sorted in registers by Batcher's odd-even
// merge network, generated at compile time for every C, on integer keys (the
// total order of the bit patterns, -0 below +0), so every index into the
// value array is a constant and nothing goes to scratch.
#include <hip/hip_runtime.h>

#include <utility>

#include "sa_compress.h"

namespace sa {
namespace flame {

using namespace sa::elems;
using namespace sa::entry;
using namespace sa::wave;

constexpr int kMaxC = SA_FLAME_MAX_CLIENTS;
// up to this many clients the Gram matrix (C (C + 1) / 2 accumulators) stays
// beside the tile in one pass; above, its rows are split over two passes
// (DESIGN.md §19 has the resource report this was decided by)
constexpr int kFusedClients = 8;

// the kernels' by-value arguments: no device allocation holds the pointer table
struct Ptrs {
  const void* p[kMaxC];
};
struct CombineArgs {
  const void* p[kMaxC];
  double s[kMaxC], w[kMaxC];
};

__host__ __device__ constexpr int gram_count(int c) { return c * (c + 1) / 2; }
__host__ __device__ constexpr int stat_count(int c) { return gram_count(c) + c; }
// the slot of G[i][i] in the packed upper triangle (row-major, j >= i)
__host__ __device__ constexpr int row_slot(int c, int i) { return i * c - i * (i - 1) / 2; }
// the rows the first pass takes: all of them up to kFusedClients, else about
// half of the matrix's entries
__host__ __device__ constexpr int first_rows(int c) {
  if (c <= kFusedClients) return c;
  int r = 0, have = 0;
  while (2 * have < gram_count(c)) have += c - r, r++;
  return r;
}

// --- the order: integer keys --------------------------------------------------
template <class T>
struct Key;
template <>
struct Key<float> {
  typedef int32_t type;
  static constexpr int32_t kMag = 0x7fffffff;
};
template <>
struct Key<double> {
  typedef int64_t type;
  static constexpr int64_t kMag = 0x7fffffffffffffffll;
};

// the bit pattern as a signed integer whose order is the values' order with
// -0 < +0 (negative patterns have their magnitude bits flipped); its own inverse
template <class T>
__device__ __forceinline__ typename Key<T>::type to_key(T x) {
  typedef typename Key<T>::type K;
  K b;
  __builtin_memcpy(&b, &x, sizeof b);
  return b ^ ((b >> (8 * (int)sizeof(K) - 1)) & Key<T>::kMag);
}
template <class T>
__device__ __forceinline__ T from_key(typename Key<T>::type k) {
  typedef typename Key<T>::type K;
  const K b = k ^ ((k >> (8 * (int)sizeof(K) - 1)) & Key<T>::kMag);
  T x;
  __builtin_memcpy(&x, &b, sizeof x);
  return x;
}

// --- the sorting network --------------------------------------------------------
// Batcher's odd-even merge sort of C values as a list of compare-exchanges
// (lo, hi), lo < hi: the network of the next power of two without the
// exchanges that touch an index >= C (those values would be +infinity and
// never move).  63 exchanges at C = 16.
constexpr int kMaxExchanges = 64;
struct Net {
  int n;
  int lo[kMaxExchanges], hi[kMaxExchanges];
};
template <int C>
constexpr Net make_net() {
  Net net = {};
  for (int p = 1; p < C; p *= 2)
    for (int k = p; k >= 1; k /= 2)
      for (int j = k % p; j + k < C; j += 2 * k)
        for (int i = 0; i < k && i + j + k < C; i++)
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) net.lo[net.n] = i + j, net.hi[net.n] = i + j + k, net.n++;
  return net;
}

template <int C, class K, size_t... I>
__device__ __forceinline__ void sort_keys(K (&v)[C], std::index_sequence<I...>) {
  constexpr Net net = make_net<C>();
  auto exchange = [](K& a, K& b) {
    const K lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo, b = hi;
  };
  (exchange(v[net.lo[I]], v[net.hi[I]]), ...);
}

// the median of C values in T: the middle one, or (lo + hi) / T(2) with the add
// and the divide rounded in T; a NaN among them gives NaN
template <class T, int C>
__device__ __forceinline__ T median_of(const T (&x)[C]) {
  typedef typename Key<T>::type K;
  K k[C];
  bool nan = false;
#pragma unroll
  for (int c = 0; c < C; c++) k[c] = to_key(x[c]), nan |= x[c] != x[c];
  sort_keys<C, K>(k, std::make_index_sequence<make_net<C>().n>());
  T g;
  if constexpr (C % 2) {
    g = from_key<T>(k[C / 2]);
  } else {
    const T s = from_key<T>(k[C / 2 - 1]) + from_key<T>(k[C / 2]);
    g = s / T(2);
  }
  return nan ? T(__builtin_nan("")) : g;
}

// --- the statistics pass -----------------------------------------------------------
// Rows [RLO, RHI) of the Gram matrix (entries j >= i), and with MED the median
// and the N[i]; clients below RLO are not read without MED.  A lane's
// elements past the tensor's end are zeros in every client: they add nothing.
// partial[block * S + slot], S = stat_count(C): this pass's slots of every block.
template <class T, int C, int RLO, int RHI, bool MED>
__global__ void __launch_bounds__(kBlock) k_stats(const Ptrs px, uint64_t n, uint64_t len, int vec,
                                                  T* __restrict__ g_out, double* __restrict__ partial) {
  constexpr int kFirst = MED ? 0 : RLO;
  constexpr int NG = row_slot(C, RHI) - row_slot(C, RLO), NN = MED ? C : 0, NA = NG + NN;
  __shared__ double ws[kWaves][NA];
  double acc[NA];
#pragma unroll
  for (int a = 0; a < NA; a++) acc[a] = 0.0;
  const Range w = wave_range(n, len);
  for (uint64_t t = w.lo; t < w.hi; t += kTile) {
    const uint64_t e0 = t + (uint64_t)w.lane * kEpl;
    const int cnt = lane_count(e0, w.hi);
    Elems<T> x[C];
#pragma unroll
    for (int c = kFirst; c < C; c++) x[c] = load_elems(reinterpret_cast<const T*>(px.p[c]), e0, cnt, vec);
    Elems<T> gv;
#pragma unroll
    for (int e = 0; e < kEpl; e++) {
      if constexpr (MED) {
        T v[C];
#pragma unroll
        for (int c = 0; c < C; c++) v[c] = x[c].v[e];
        const T g = median_of<T, C>(v);
        gv.v[e] = g;
#pragma unroll
        for (int c = 0; c < C; c++) {
          const double d = (double)(v[c] - g);  // the difference rounds in T
          acc[NG + c] = fma(d, d, acc[NG + c]);
        }
      }
      double xd[C];
#pragma unroll
      for (int c = kFirst; c < C; c++) xd[c] = (double)x[c].v[e];
      int a = 0;
#pragma unroll
      for (int i = RLO; i < RHI; i++) {
#pragma unroll
        for (int j = i; j < C; j++, a++) acc[a] = fma(xd[i], xd[j], acc[a]);
      }
    }
    if constexpr (MED) store_elems(g_out, e0, cnt, vec, gv);
  }
  // the wave's sums by a fixed butterfly, then the block's in wave order
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < NA; a++) {
    double v = acc[a];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (w.lane == 0) ws[wave][a] = v;
  }
  __syncthreads();
  constexpr int S = stat_count(C);
  for (int a = threadIdx.x; a < NA; a += kBlock) {
    double v = ws[0][a];
    for (int i = 1; i < kWaves; i++) v += ws[i][a];
    const int slot = a < NG ? row_slot(C, RLO) + a : gram_count(C) + (a - NG);
    partial[(uint64_t)blockIdx.x * S + slot] = v;
  }
}

// one block: stats[s] (+)= the blocks' partials of slot s, in block order
__global__ void __launch_bounds__(kBlock) k_join(const double* __restrict__ partial, int nblocks, int S,
                                                 double* __restrict__ stats, int accumulate) {
  for (int s = threadIdx.x; s < S; s += kBlock) {
    double v = 0.0;
    for (int b = 0; b < nblocks; b++) v += partial[(uint64_t)b * S + s];
    stats[s] = accumulate ? stats[s] + v : v;
  }
}

// --- the combine pass ----------------------------------------------------------------
// out = (sum over the K kept clients, in order, of float64(g + (x_i - g) s_i) w_i) / W + 0.0;
// every operation of m_i rounds in T, the multiply and the add of the sum round
// separately (nothing is contracted: the reference is numpy)
template <class T, int K>
__global__ void __launch_bounds__(kBlock) k_combine(const CombineArgs a, uint64_t n, uint64_t len, int vec,
                                                    const T* __restrict__ g, double divisor,
                                                    double* __restrict__ out) {
#pragma clang fp contract(off)
  const Range w = wave_range(n, len);
  T s[K];
#pragma unroll
  for (int c = 0; c < K; c++) s[c] = (T)a.s[c];
  for (uint64_t t = w.lo; t < w.hi; t += kTile) {
    const uint64_t e0 = t + (uint64_t)w.lane * kEpl;
    const int cnt = lane_count(e0, w.hi);
    Elems<T> x[K];
#pragma unroll
    for (int c = 0; c < K; c++) x[c] = load_elems(reinterpret_cast<const T*>(a.p[c]), e0, cnt, vec);
    const Elems<T> gv = load_elems(g, e0, cnt, vec);
    Elems<double> r;
#pragma unroll
    for (int e = 0; e < kEpl; e++) {
      double sum = 0.0;
#pragma unroll
      for (int c = 0; c < K; c++) {
        const T d = x[c].v[e] - gv.v[e];
        const T m = gv.v[e] + d * s[c];
        const double p = (double)m * a.w[c];
        sum = sum + p;
      }
      const double q = sum / divisor;
      r.v[e] = q + 0.0;
    }
    store_elems(out, e0, cnt, vec, r);
  }
}

// --- launches ----------------------------------------------------------------------------
template <class T, int C>
static void launch_stats(const Ptrs& px, uint64_t n, const Grid& g, void* median_out, double* partial,
                         hipStream_t st) {
  constexpr int R = first_rows(C);
  hipLaunchKernelGGL((k_stats<T, C, 0, R, true>), dim3(g.grid), dim3(kBlock), 0, st, px, n, g.len, g.vec,
                     (T*)median_out, partial);
  if constexpr (R < C)
    hipLaunchKernelGGL((k_stats<T, C, R, C, false>), dim3(g.grid), dim3(kBlock), 0, st, px, n, g.len, g.vec,
                       (T*)median_out, partial);
}

template <class T, int K>
static void launch_combine(const CombineArgs& a, uint64_t n, const Grid& g, const void* median, double divisor,
                           double* out, hipStream_t st) {
  hipLaunchKernelGGL((k_combine<T, K>), dim3(g.grid), dim3(kBlock), 0, st, a, n, g.len, g.vec, (const T*)median,
                     divisor, out);
}

// f(std::integral_constant<int, c>()) for c in 1 .. kMaxC (checked before)
template <class F>
static void dispatch_clients(int c, F&& f) {
#define SA_FLAME_CASE(N) \
  case N:                \
    f(std::integral_constant<int, N>()); \
    break;
  switch (c) {
    SA_FLAME_CASE(1) SA_FLAME_CASE(2) SA_FLAME_CASE(3) SA_FLAME_CASE(4) SA_FLAME_CASE(5) SA_FLAME_CASE(6)
    SA_FLAME_CASE(7) SA_FLAME_CASE(8) SA_FLAME_CASE(9) SA_FLAME_CASE(10) SA_FLAME_CASE(11) SA_FLAME_CASE(12)
    SA_FLAME_CASE(13) SA_FLAME_CASE(14) SA_FLAME_CASE(15) SA_FLAME_CASE(16)
  }
#undef SA_FLAME_CASE
}

static int check_clients(int n_clients, const char* what) {
  if (n_clients < 1 || n_clients > kMaxC) {
    sa_set_error("%s: n_clients must be in 1..%d (SA_FLAME_MAX_CLIENTS)", what, kMaxC);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

}  // namespace flame
}  // namespace sa

using namespace sa::flame;

extern "C" int sa_flame_scratch_bytes(uint64_t n, int n_clients, int x_type) {
  int rc = check_float_n(x_type, n, 32, "sa_flame_scratch_bytes");
  if (rc == SA_OK) rc = check_clients(n_clients, "sa_flame_scratch_bytes");
  if (rc != SA_OK) return rc;
  return (int)(wave_grid(n, 0).grid * stat_count(n_clients) * sizeof(double));
}

extern "C" int sa_flame_stats(const void* const* x, int n_clients, int x_type, uint64_t n, void* median_out,
                              void* scratch, double* stats, int accumulate, void* stream) {
  int rc = check_float_n(x_type, n, 32, "sa_flame_stats");
  if (rc == SA_OK) rc = check_clients(n_clients, "sa_flame_stats");
  if (rc != SA_OK) return rc;
  const uintptr_t esz = elem_size(x_type);
  if (!stats || misaligned(stats, 8)) {
    sa_set_error("sa_flame_stats: bad arguments (stats is required, 8-byte aligned)");
    return SA_ERR_ARG;
  }
  const int S = stat_count(n_clients);
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {  // nothing to add; a store is a store of zeros
    if (!accumulate) SA_HIP_CHECK(hipMemsetAsync(stats, 0, S * sizeof(double), st));
    return SA_OK;
  }
  if (!x || !median_out || !scratch || misaligned(median_out, esz) || misaligned(scratch, 8)) {
    sa_set_error("sa_flame_stats: bad arguments (x, median_out and scratch are required; element-aligned "
                 "median_out, 8-byte aligned scratch)");
    return SA_ERR_ARG;
  }
  Ptrs px = {};
  uintptr_t ptrs = (uintptr_t)median_out;
  for (int c = 0; c < n_clients; c++) {
    if (!x[c] || misaligned(x[c], esz)) {
      sa_set_error("sa_flame_stats: bad arguments (client %d's tensor is required, element-aligned)", c);
      return SA_ERR_ARG;
    }
    px.p[c] = x[c], ptrs |= (uintptr_t)x[c];
  }
  const Grid g = wave_grid(n, ptrs);
  dispatch_float(x_type, [&](auto t) {
    typedef decltype(t) T;
    dispatch_clients(n_clients, [&](auto c) { launch_stats<T, decltype(c)::value>(px, n, g, median_out, (double*)scratch, st); });
  });
  hipLaunchKernelGGL(k_join, dim3(1), dim3(kBlock), 0, st, (const double*)scratch, g.grid, S, stats, accumulate);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_flame_combine(const void* const* x, const double* scale, const double* weight, int n_clients,
                                int x_type, uint64_t n, const void* median, double divisor, double* out,
                                void* stream) {
  int rc = check_float_n(x_type, n, 32, "sa_flame_combine");
  if (rc == SA_OK) rc = check_clients(n_clients, "sa_flame_combine");
  if (rc != SA_OK) return rc;
  const uintptr_t esz = elem_size(x_type);
  if (!x || !scale || !weight) {
    sa_set_error("sa_flame_combine: bad arguments (x, scale and weight are required)");
    return SA_ERR_ARG;
  }
  // a dropped client (its weight is a NaN) is left out here: its pointer never reaches the kernel
  CombineArgs a = {};
  uintptr_t ptrs = (uintptr_t)median | (uintptr_t)out;
  int kept = 0;
  for (int c = 0; c < n_clients; c++) {
    if (weight[c] != weight[c]) continue;
    if (n && (!x[c] || misaligned(x[c], esz))) {
      sa_set_error("sa_flame_combine: bad arguments (client %d's tensor is required, element-aligned)", c);
      return SA_ERR_ARG;
    }
    a.p[kept] = x[c], a.s[kept] = scale[c], a.w[kept] = weight[c], ptrs |= (uintptr_t)x[c];
    kept++;
  }
  if (kept == 0) {
    sa_set_error("sa_flame_combine: every client is dropped (a NaN weight drops a client)");
    return SA_ERR_ARG;
  }
  if (n == 0) return SA_OK;
  if (!median || !out || misaligned(median, esz) || misaligned(out, 8)) {
    sa_set_error("sa_flame_combine: bad arguments (median and out are required; element-aligned median, 8-byte "
                 "aligned out)");
    return SA_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const Grid g = wave_grid(n, ptrs);
  dispatch_float(x_type, [&](auto t) {
    typedef decltype(t) T;
    dispatch_clients(kept, [&](auto c) { launch_combine<T, decltype(c)::value>(a, n, g, median, divisor, out, st); });
  });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}
