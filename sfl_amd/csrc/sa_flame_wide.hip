// sa_flame_wide.hip — FlameAggregator's per-element work for 17 to 64 clients
// (SA_FLAME_WIDE_MAX_CLIENTS; sa_flame.hip serves 1 to 16 with one lane an
// element and the client count a template argument, which stops scaling
// there: DESIGN.md §19, "More than 16 clients").  The definition is
// sa_flame.hip's (include/sfl_sa.h); the work is split differently:
//
//   k_stats_wide  a block of four waves per tile of kE elements, looping over
//             its tiles.  The C clients' rows of a tile are staged once in LDS
//             (CP rows, CP = 32 or 64 the padded client count; rows C .. CP - 1
//             are zeros that only LDS holds), and everything reads them there:
//             - the Gram matrix on v_mfma_f64_16x16x4_f64: the upper-triangle
//               16 x 16 tiles of CP x CP (3 or 10), each wave a quarter of the
//               tile's elements as the k dimension, accumulators in registers
//               over all of the block's tiles;
//             - the median: one thread an element, the CP keys in registers,
//               Batcher's network pruned to the two middle outputs; the pads
//               are sentinel keys, so many below and so many above the real
//               values that the real values' middle lands at CP/2 - 1, CP/2;
//             - N[i]: wave w owns clients w, w + 4, ..., its lanes walk the
//               tile's columns.
//             A block adds its waves' sums in wave order and writes one partial.
//   k_join_wide   one thread a statistic: the blocks' partials in block order,
//             into the packed layout of the actual C.
//   k_combine_wide  one streaming pass in sa_compress.h's wave layout with a
//             run-time loop over the kept clients, kInFlight clients' loads
//             in flight; sa_flame.hip's arithmetic, operation for operation.
//
// The grids are functions of n only and there are no atomics: the same input
// gives the same bits.
#include <hip/hip_runtime.h>

#include <utility>

#include "sa_compress.h"
#include "sa_flame_keys.h"

namespace sa {
namespace flame_wide {

using namespace sa::elems;
using namespace sa::entry;
using namespace sa::flame;
using namespace sa::wave;

typedef double double4 __attribute__((ext_vector_type(4)));  // the matrix instruction's accumulator

constexpr int kMaxC = SA_FLAME_WIDE_MAX_CLIENTS;
constexpr int kE = 128;                 // elements a tile
constexpr int kCols = kE / kWaves;      // a wave's share of a tile's k dimension
constexpr int kStatBlocks = 512;        // 2 resident blocks per CU on 256 CUs
// LDS row stride in elements.  A lane (i = lane % 16, g = lane / 16) reads
// the four consecutive elements of row 16 t + i at column k0 + 4 g as one
// operand fetch.  float32: the stride is 132 words = 4 mod 64 banks, so the 16
// lanes of a lane group start 4 banks apart and their 16-byte pieces tile the
// 64 banks once.  float64: 264 words = 8 mod 64, so 8 lanes' 32-byte pieces
// tile the banks once and a lane group takes the two passes its 512 bytes
// need anyway.  The staging stores, the median's column reads and N's reads
// have consecutive lanes at consecutive elements of one row: no conflicts at
// any stride.  Rows stay 16-byte aligned (132 * 4 = 16 * 33).
constexpr int kLd = kE + 4;
constexpr int kInFlight = 8;            // the combine: clients whose loads are in flight together

static_assert(kCols % 16 == 0 && kE % 64 == 0, "a wave takes whole 16-column operand fetches");

__host__ __device__ constexpr int padded(int c) { return c <= 32 ? 32 : 64; }
__host__ __device__ constexpr int tile_count(int cp) { return (cp / 16) * (cp / 16 + 1) / 2; }
// a block's partial: the Gram tiles as the instruction leaves them (tile q,
// register r, lane: [q * 256 + r * 64 + lane]), then CP values of N
__host__ __device__ constexpr int partial_count(int cp) { return tile_count(cp) * 256 + cp; }

typedef ClientPtrs<kMaxC> Ptrs;
struct CombineArgs : ClientArgs<kMaxC> {
  int kept;  // the clients are a run-time loop here
};

// the launch of the statistics pass: a function of n only
struct StatGrid {
  uint32_t tiles, per_block, grid;
};
inline StatGrid stat_grid(uint64_t n) {
  StatGrid g;
  g.tiles = (uint32_t)((n + kE - 1) / kE);
  g.per_block = (g.tiles + kStatBlocks - 1) / kStatBlocks;
  g.grid = g.per_block ? (g.tiles + g.per_block - 1) / g.per_block : 0;
  return g;
}

// --- the sorting network --------------------------------------------------------
// sa_flame_keys.h's network of CP values (a power of two) without the
// exchanges from which neither middle output (CP/2 - 1, CP/2) can be reached,
// filled up to a multiple of kChunk with exchanges of value 0 with itself
// (nothing).  543 exchanges at CP = 64, 191 at 32, before the pruning.
constexpr int kChunk = 64;
template <int CP>
constexpr Net make_net() {
  const Net all = batcher<CP>();
  bool need[CP] = {}, keep[kMaxExchanges] = {};
  need[CP / 2 - 1] = need[CP / 2] = true;
  for (int q = all.n - 1; q >= 0; q--)
    if (need[all.lo[q]] || need[all.hi[q]]) keep[q] = need[all.lo[q]] = need[all.hi[q]] = true;
  Net net = {};
  for (int q = 0; q < all.n; q++)
    if (keep[q]) net.lo[net.n] = all.lo[q], net.hi[net.n] = all.hi[q], net.n++;
  while (net.n % kChunk) net.lo[net.n] = net.hi[net.n] = 0, net.n++;
  return net;
}

// kChunk exchanges from B on: every index is a constant
template <int CP, int B, class K, size_t... I>
__device__ __forceinline__ void sort_chunk(K (&v)[CP], std::index_sequence<I...>) {
  constexpr Net net = make_net<CP>();
  auto exchange = [](K& a, K& b) {
    const K lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo, b = hi;
  };
  (exchange(v[net.lo[B + I]], v[net.hi[B + I]]), ...);
}
template <int CP, class K, size_t... B>
__device__ __forceinline__ void sort_keys(K (&v)[CP], std::index_sequence<B...>) {
  (sort_chunk<CP, kChunk * (int)B, K>(v, std::make_index_sequence<kChunk>()), ...);
}

// The median of the C real values of one column (x[c * kLd], c < C) in T.
// Rows C .. CP - 1 get sentinel keys: n_low of them the smallest key, the rest
// the largest.  With n_low = CP/2 - 1 - (C - 1) / 2 the sorted real values
// stand at n_low .. n_low + C - 1, so their lower middle (C - 1) / 2 is at
// CP/2 - 1, and for even C the upper middle C / 2 = (C - 1) / 2 + 1 at CP/2;
// the pads above number CP - C - n_low >= 0 because (C - 1) / 2 <= CP/2 - 1.
// The sentinels are NaN bit patterns; a real NaN may tie with one, and a NaN
// among the real values overrides the result anyway.
template <class T, int CP>
__device__ __forceinline__ T median_col(const T* x, int C, int n_low, bool odd) {
  typedef typename Key<T>::type K;
  constexpr K kLow = (K)((uint64_t)1 << (8 * sizeof(K) - 1)), kHigh = ~kLow;
  K k[CP];
  bool nan = false;
#pragma unroll
  for (int c = 0; c < CP; c++) {
    const T v = x[c * kLd];
    const bool real = c <= CP / 2 || c < C;  // (C > CP/2 always)
    nan |= real && v != v;
    k[c] = real ? to_key(v) : (c - C < n_low ? kLow : kHigh);
  }
  sort_keys<CP, K>(k, std::make_index_sequence<make_net<CP>().n / kChunk>());
  const T lo = from_key<T>(k[CP / 2 - 1]), hi = from_key<T>(k[CP / 2]);
  const T s = lo + hi;
  const T g = odd ? lo : s / T(2);
  return nan ? T(__builtin_nan("")) : g;
}

template <class T>
struct Vec16;
template <>
struct Vec16<float> {
  typedef f32x4 type;
};
template <>
struct Vec16<double> {
  typedef f64x2 type;
};

// the four consecutive elements at p (16-byte aligned, LDS) as float64
__device__ __forceinline__ void operand4(const float* p, double (&a)[4]) {
  const f32x4 v = *reinterpret_cast<const f32x4*>(p);
  a[0] = (double)v.x, a[1] = (double)v.y, a[2] = (double)v.z, a[3] = (double)v.w;
}
__device__ __forceinline__ void operand4(const double* p, double (&a)[4]) {
  const f64x2 v0 = *reinterpret_cast<const f64x2*>(p), v1 = *reinterpret_cast<const f64x2*>(p + 2);
  a[0] = v0.x, a[1] = v0.y, a[2] = v1.x, a[3] = v1.y;
}

// --- the statistics pass -----------------------------------------------------------
// Block b owns tiles [b * per_block, (b + 1) * per_block) of kE elements.
// partial[b * partial_count(CP) + ...]: see partial_count.
template <class T, int CP>
__global__ void __launch_bounds__(kBlock) k_stats_wide(const Ptrs px, int C, uint64_t n, uint32_t tiles,
                                                       uint32_t per_block, int vec, T* __restrict__ g_out,
                                                       double* __restrict__ partial) {
  constexpr int NT = CP / 16, NG = tile_count(CP), NQ = CP / kWaves;
  typedef typename Vec16<T>::type V;
  constexpr int VE = 16 / (int)sizeof(T), CPR = kE / VE;  // elements a 16-byte piece, pieces a row
  static_assert(NG * 256 * sizeof(double) <= CP * kLd * sizeof(T), "the waves' sums are joined in the rows' LDS");
  __shared__ __attribute__((aligned(16))) T xs[CP * kLd];
  __shared__ T gl[kE];
  __shared__ const T* ptab[CP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < CP) ptab[tid] = tid < C ? reinterpret_cast<const T*>(px.p[tid]) : nullptr;
  for (int i = C * kLd + tid; i < CP * kLd; i += kBlock) xs[i] = T(0);  // the pad rows, once

  double4 acc[NG];
#pragma unroll
  for (int q = 0; q < NG; q++) acc[q] = double4{0, 0, 0, 0};
  double nacc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; q++) nacc[q] = 0.0;
  const int n_low = CP / 2 - 1 - (C - 1) / 2;
  const bool odd = C & 1;

  const uint32_t t0 = blockIdx.x * per_block, t1 = t0 + per_block < tiles ? t0 + per_block : tiles;
  for (uint32_t t = t0; t < t1; t++) {
    const uint64_t e0 = (uint64_t)t * kE;
    const int cnt = n - e0 < (uint64_t)kE ? (int)(n - e0) : kE;
    __syncthreads();  // the last tile's readers are done (and the table and the pads are written)
    // the C rows of the tile into LDS; columns past the tensor's end are zeros
    if (vec && cnt == kE) {
      const int pieces = C * CPR;
      for (int i0 = tid; i0 < pieces; i0 += 4 * kBlock) {
        V v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int i = i0 + j * kBlock;
          if (i < pieces) v[j] = *reinterpret_cast<const V*>(ptab[i / CPR] + e0 + (i % CPR) * VE);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int i = i0 + j * kBlock;
          if (i < pieces) *reinterpret_cast<V*>(&xs[(i / CPR) * kLd + (i % CPR) * VE]) = v[j];
        }
      }
    } else {
      for (int i = tid; i < C * kE; i += kBlock) {
        const int row = i / kE, col = i % kE;
        xs[row * kLd + col] = col < cnt ? ptab[row][e0 + col] : T(0);
      }
    }
    __syncthreads();
    // the Gram matrix: this wave's kCols columns, 16 a fetch; step s of a fetch has lane group g at column 4 g + s
#pragma unroll
    for (int h = 0; h < kCols / 16; h++) {
      const int col = wave * kCols + 16 * h + 4 * (lane >> 4);
      double a[NT][4];
#pragma unroll
      for (int r = 0; r < NT; r++) operand4(&xs[(16 * r + (lane & 15)) * kLd + col], a[r]);
#pragma unroll
      for (int s = 0; s < 4; s++) {
        int q = 0;
#pragma unroll
        for (int ra = 0; ra < NT; ra++)
#pragma unroll
          for (int rb = ra; rb < NT; rb++, q++)
            acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ra][s], a[rb][s], acc[q], 0, 0, 0);
      }
    }
    // the median: one thread a column
    if (tid < kE) {
      T g = T(0);
      if (tid < cnt) {
        g = median_col<T, CP>(xs + tid, C, n_low, odd);
        g_out[e0 + tid] = g;
      }
      gl[tid] = g;
    }
    __syncthreads();
    // N: (a column past the end has x = g = 0 and adds +0)
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const int c = wave + kWaves * q;
      if (c < C) {
#pragma unroll
        for (int j = 0; j < kE / 64; j++) {
          const int col = lane + 64 * j;
          const double d = (double)(xs[c * kLd + col] - gl[col]);  // the difference rounds in T
          nacc[q] = fma(d, d, nacc[q]);
        }
      }
    }
  }
  // the block's Gram tiles: the waves' accumulators in wave order, through the rows' LDS
  __syncthreads();
  double* buf = reinterpret_cast<double*>(xs);
  double* mine = partial + (uint64_t)blockIdx.x * partial_count(CP);
  for (int w = 0; w < kWaves; w++) {
    if (wave == w) {
#pragma unroll
      for (int q = 0; q < NG; q++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int at = q * 256 + r * 64 + lane;
          const double v = w ? buf[at] + acc[q][r] : acc[q][r];
          if (w == kWaves - 1)
            mine[at] = v;
          else
            buf[at] = v;
        }
      }
    }
    __syncthreads();
  }
  // N: a client has one wave; its lanes by a fixed butterfly (the pads' sums are zeros)
#pragma unroll
  for (int q = 0; q < NQ; q++) {
    double v = nacc[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) mine[NG * 256 + wave + kWaves * q] = v;
  }
}

// one thread a statistic of the actual C: stats[s] (+)= the blocks' partials of
// its place, in block order.  G[i][j] is element (i % 16, j % 16) of tile
// (i / 16, j / 16), which the instruction leaves in register row / 4 of lane
// 16 (row % 4) + col.
__global__ void __launch_bounds__(kBlock) k_join_wide(const double* __restrict__ partial, int nblocks, int C, int CP,
                                                      double* __restrict__ stats, int accumulate) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= stat_count(C)) return;
  const int NT = CP / 16, NG = tile_count(CP), PS = partial_count(CP);
  int at;
  if (s < gram_count(C)) {
    int i = 0;
    while (s >= row_slot(C, i + 1)) i++;
    const int j = i + s - row_slot(C, i);
    const int ra = i >> 4, rb = j >> 4, q = ra * NT - ra * (ra - 1) / 2 + (rb - ra), row = i & 15, col = j & 15;
    at = q * 256 + (row >> 2) * 64 + (row & 3) * 16 + col;
  } else {
    at = NG * 256 + (s - gram_count(C));
  }
  double v = 0.0;
  for (int b = 0; b < nblocks; b++) v += partial[(uint64_t)b * PS + at];
  stats[s] = accumulate ? stats[s] + v : v;
}

// --- the combine pass ----------------------------------------------------------------
// sa_flame.hip's k_combine with the kept clients as a run-time loop, in client
// order: every operation of m_i rounds in T, the multiply and the add of the
// sum round separately, nothing is contracted
template <class T>
__global__ void __launch_bounds__(kBlock) k_combine_wide(const CombineArgs a, uint64_t n, uint64_t len, int vec,
                                                         const T* __restrict__ g, double divisor,
                                                         double* __restrict__ out) {
#pragma clang fp contract(off)
  const Range w = wave_range(n, len);
  for (uint64_t t = w.lo; t < w.hi; t += kTile) {
    const uint64_t e0 = t + (uint64_t)w.lane * kEpl;
    const int cnt = lane_count(e0, w.hi);
    const Elems<T> gv = load_elems(g, e0, cnt, vec);
    double sum[kEpl];
#pragma unroll
    for (int e = 0; e < kEpl; e++) sum[e] = 0.0;
    for (int c0 = 0; c0 < a.kept; c0 += kInFlight) {
      Elems<T> x[kInFlight];
#pragma unroll
      for (int j = 0; j < kInFlight; j++)
        if (c0 + j < a.kept) x[j] = load_elems(reinterpret_cast<const T*>(a.p[c0 + j]), e0, cnt, vec);
#pragma unroll
      for (int j = 0; j < kInFlight; j++) {
        if (c0 + j < a.kept) {
          const T s = (T)a.s[c0 + j];
          const double wt = a.w[c0 + j];
#pragma unroll
          for (int e = 0; e < kEpl; e++) {
            const T d = x[j].v[e] - gv.v[e];
            const T m = gv.v[e] + d * s;
            const double p = (double)m * wt;
            sum[e] = sum[e] + p;
          }
        }
      }
    }
    Elems<double> r;
#pragma unroll
    for (int e = 0; e < kEpl; e++) {
      const double q = sum[e] / divisor;
      r.v[e] = q + 0.0;
    }
    store_elems(out, e0, cnt, vec, r);
  }
}

}  // namespace flame_wide
}  // namespace sa

using namespace sa::flame_wide;

extern "C" int sa_flame_wide_scratch_bytes(uint64_t n, int n_clients, int x_type) {
  const int rc = check_scalars(x_type, n, n_clients, kWide, "sa_flame_wide_scratch_bytes");
  if (rc != SA_OK) return rc;
  return (int)(stat_grid(n).grid * partial_count(padded(n_clients)) * sizeof(double));
}

extern "C" int sa_flame_stats_wide(const void* const* x, int n_clients, int x_type, uint64_t n, void* median_out,
                                   void* scratch, double* stats, int accumulate, void* stream) {
  Ptrs px = {};
  uintptr_t ptrs = 0;
  const int rc = check_stats(x, n_clients, x_type, n, median_out, scratch, stats, kWide, "sa_flame_stats_wide", px.p,
                             &ptrs);
  if (rc != SA_OK) return rc;
  const int CP = padded(n_clients), S = stat_count(n_clients);
  const StatGrid g = stat_grid(n);
  hipStream_t st = (hipStream_t)stream;
  if (n == 0 && accumulate) return SA_OK;  // nothing to add
  if (n)
    dispatch_float(x_type, [&](auto t) {
      typedef decltype(t) T;
      auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(kBlock), 0, st, px, n_clients, n, g.tiles, g.per_block,
                           (int)((ptrs & 15) == 0), (T*)median_out, (double*)scratch);
      };
      if (CP == 32)
        launch(k_stats_wide<T, 32>);
      else
        launch(k_stats_wide<T, 64>);
    });
  // (n == 0: no partials, a store of zeros by the same kernel)
  hipLaunchKernelGGL(k_join_wide, dim3((S + kBlock - 1) / kBlock), dim3(kBlock), 0, st, (const double*)scratch,
                     (int)g.grid, n_clients, CP, stats, accumulate);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_flame_combine_wide(const void* const* x, const double* scale, const double* weight, int n_clients,
                                     int x_type, uint64_t n, const void* median, double divisor, double* out,
                                     void* stream) {
  CombineArgs a = {};
  uintptr_t ptrs = (uintptr_t)median | (uintptr_t)out;
  const int rc = check_combine(x, scale, weight, n_clients, x_type, n, median, out, kWide, "sa_flame_combine_wide", &a,
                               &a.kept, &ptrs);
  if (rc != SA_OK || n == 0) return rc;
  hipStream_t st = (hipStream_t)stream;
  const Grid g = wave_grid(n, ptrs);
  dispatch_float(x_type, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL(k_combine_wide<T>, dim3(g.grid), dim3(kBlock), 0, st, a, n, g.len, g.vec, (const T*)median,
                       divisor, out);
  });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}
