// sa_mars.hip — the feature extraction of MarsAggregator on the device (the
// reference's Lipschitz-based robust aggregator, examples/security/h_bd/
// agg_mars.py:27-153; sfl_amd/security/aggregation/mars_aggregator.py has the
// definition and the host form, DESIGN.md §22 the split and the LDS use):
//
//   sigma = the largest singular value of every rows x cols matrix of one
//           layer of all clients, in float64, times the following
//           BatchNorm's scale where there is one
//   bn    = |w| / sqrt(max(var, 0) + 1e-5) for every BatchNorm channel
//
// sigma: one wave, alone in its block, per (client, matrix); the grid is a
// function of the shapes only.  With p = min(rows, cols) <= 32 and K =
// max(rows, cols) the wave
//   1. forms the p x p Gram matrix X X^T of the p x K matrix X (X = W for
//      rows < cols, X = W^T otherwise: one accumulate body, two strides) on
//      zero-padded 16-wide tiles with v_mfma_f64_16x16x4_f64.  Both operands
//      of a tile on the diagonal are the same register: lane l holds
//      X[l % 16][k + l / 16] as A's element (row l % 16, column l / 16) and as
//      B's element (row l / 16, column l % 16).  p <= 16 takes one tile,
//      p <= 32 three of the four (the fourth by symmetry).  A lane group takes
//      four consecutive k, one per MFMA, so that along a contiguous K the
//      wave reads 16 consecutive elements of a row; the order of the k of a
//      sum is fixed by that and is the same on every run.
//   2. writes the tiles into a p x p matrix in LDS (stride 33 doubles, 8.3 KB)
//      and diagonalises it by cyclic Jacobi in a round-robin order: q - 1
//      rounds a sweep (q = p rounded up to even) of q / 2 disjoint rotations;
//      a round computes its rotations (one lane each), applies them to the
//      columns, then to the rows, (pair, index) items spread over the lanes.
//      A rotated pair's off-diagonal element is stored as zero and its
//      diagonal by the update formula, so off-diagonal elements shrink
//      relatively and the loop's test can be met.
//   3. stops when sum offdiag^2 <= 2^-104 trace^2 or after kMaxSweeps sweeps,
//      whichever is first, and stores sqrt(max(largest diagonal, 0)) * scale.
// A non-finite trace (a NaN or an infinity in the matrix, or an overflowing
// square) skips the sweeps: the value is sqrt(trace), NaN or +inf.
// No atomics, no data-dependent grid: the same input gives the same bits.
#include <hip/hip_runtime.h>

#include "sa_compress.h"

namespace sa {
namespace mars {

using namespace sa::entry;

constexpr int kMaxC = SA_FLAME_MAX_CLIENTS;
constexpr int kMaxP = SA_MARS_MAX_P;
constexpr int kWave = 64;
constexpr int kLd = kMaxP + 1;  // the LDS matrix's row stride: rows two banks apart
constexpr int kMaxSweeps = 30;
constexpr double kEps = 1e-5;  // the BatchNorm epsilon of agg_mars.py:94 and :119

typedef double double4 __attribute__((ext_vector_type(4)));

// the kernels' by-value arguments: no device allocation holds the pointer tables
struct Ptrs {
  const void* w[kMaxC];
  const void* bn_w[kMaxC];
  const void* bn_var[kMaxC];
};

template <class T>
__device__ __forceinline__ double bn_scale(const T* __restrict__ w, const T* __restrict__ var, uint64_t ch) {
  const double v = (double)var[ch];
  return fabs((double)w[ch]) / sqrt((v > 0.0 ? v : 0.0) + kEps);  // (a NaN variance is no > 0: its scale is finite)
}

// the wave's sum in a fixed butterfly: every lane gets it
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// --- the Gram matrix ------------------------------------------------------------
// X[i][k] = x[i * si + k * sk], zero outside p x K
template <class T>
__device__ __forceinline__ double x_at(const T* __restrict__ x, uint64_t i, uint64_t k, int p, uint64_t K, uint64_t si,
                                       uint64_t sk) {
  return i < (uint64_t)p && k < K ? (double)x[i * si + k * sk] : 0.0;
}

#ifndef SA_MARS_GRAM_VALU
// TILES = 1: p <= 16; TILES = 2: p <= 32.  G (LDS) gets the p x p matrix.
template <class T, int TILES>
__device__ __forceinline__ void gram(const T* __restrict__ x, int p, uint64_t K, uint64_t si, uint64_t sk, double* G,
                                     double*) {
  const int lane = threadIdx.x, i = lane & 15, g = lane >> 4;
  double4 d00 = {0, 0, 0, 0}, d01 = {0, 0, 0, 0}, d11 = {0, 0, 0, 0};
  for (uint64_t k0 = 0; k0 < K; k0 += 16) {
    double a0[4], a1[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
      a0[s] = x_at(x, i, k0 + 4 * g + s, p, K, si, sk);
      if constexpr (TILES == 2) a1[s] = x_at(x, 16 + i, k0 + 4 * g + s, p, K, si, sk);
    }
#pragma unroll
    for (int s = 0; s < 4; s++) {
      d00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[s], a0[s], d00, 0, 0, 0);
      if constexpr (TILES == 2) {
        d01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[s], a1[s], d01, 0, 0, 0);
        d11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[s], a1[s], d11, 0, 0, 0);
      }
    }
  }
  // a lane's register r is the tile's element (4 r + g, i): the float64 instruction's registers are four
  // groups of one row a lane group; the upper triangle is stored on both sides
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int row = 4 * r + g, col = i;
    if (row <= col && col < p) G[row * kLd + col] = d00[r], G[col * kLd + row] = d00[r];
    if constexpr (TILES == 2) {
      if (row < p && 16 + col < p) G[row * kLd + 16 + col] = d01[r], G[(16 + col) * kLd + row] = d01[r];
      if (row <= col && 16 + col < p) G[(16 + row) * kLd + 16 + col] = d11[r], G[(16 + col) * kLd + 16 + row] = d11[r];
    }
  }
}
#else
// The other form, for the record in DESIGN.md §22 (make VARIANT=_valu
// EXTRA=-DSA_MARS_GRAM_VALU): float64 FMAs on the vector unit.  16 k of X are
// staged in LDS (xs[kk][i]); lane l owns column l % 32 of G and its rows of
// l / 32's parity, 8 or 16 accumulators.
template <class T, int TILES>
__device__ __forceinline__ void gram(const T* __restrict__ x, int p, uint64_t K, uint64_t si, uint64_t sk, double* G,
                                     double* xs) {
  constexpr int R = 8 * TILES, kW = 16 * TILES;  // accumulators a lane; staged rows
  const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
  double acc[R];
#pragma unroll
  for (int r = 0; r < R; r++) acc[r] = 0.0;
  for (uint64_t k0 = 0; k0 < K; k0 += 16) {
    for (int e = lane; e < 16 * kW; e += kWave) {
      // consecutive lanes along the contiguous dimension
      const int i = si == 1 ? e % kW : e / 16, kk = si == 1 ? e / kW : e % 16;
      xs[kk * kLd + i] = x_at(x, i, k0 + kk, p, K, si, sk);
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < 16; kk++) {
      const double xj = j < kW ? xs[kk * kLd + j] : 0.0;
#pragma unroll
      for (int r = 0; r < R; r++) acc[r] = fma(xs[kk * kLd + 2 * r + h], xj, acc[r]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int row = 2 * r + h;
    if (row < p && j < p) G[row * kLd + j] = acc[r];
  }
}
#endif

// --- the largest eigenvalue --------------------------------------------------------
struct Rot {
  int a, b;         // a < b < p, or a < 0: nothing to do
  double c, s;      // the rotation
  double daa, dbb;  // the pair's diagonal after it
};

// round `round`'s pair `m` of q players (q even): (round, q - 1) for m = 0,
// else (round + m, round - m) modulo q - 1
__device__ __forceinline__ void pair_of(int round, int m, int q, int* a, int* b) {
  const int n1 = q - 1;
  int u = m == 0 ? round : (round + m) % n1, v = m == 0 ? n1 : (round - m + n1) % n1;
  *a = u < v ? u : v, *b = u < v ? v : u;
}

// sum of squares off the diagonal and the trace, the same in every lane
__device__ __forceinline__ void measure(const double* G, int p, double* off, double* trace) {
  double o = 0.0, t = 0.0;
  for (int e = threadIdx.x; e < p * p; e += kWave) {
    const int r = e / p, c = e - r * p;
    const double v = G[r * kLd + c];
    if (r == c) t += v;
    else o = fma(v, v, o);
  }
  *off = wave_sum(o), *trace = wave_sum(t);
}

template <class T, int TILES>
__global__ void __launch_bounds__(kWave) k_sigma(const Ptrs px, uint64_t n_mat, int p, uint64_t K, uint64_t si,
                                                 uint64_t sk, uint64_t mat_elems, uint64_t n_bn,
                                                 double* __restrict__ out) {
  __shared__ double G[kMaxP * kLd];
  __shared__ Rot rot[kMaxP / 2];
#ifdef SA_MARS_GRAM_VALU
  __shared__ double xs[16 * kLd];
#else
  double* xs = nullptr;
#endif
  const uint64_t c = blockIdx.x / n_mat, m = blockIdx.x - c * n_mat;
  const int lane = threadIdx.x;
  const T* x = reinterpret_cast<const T*>(px.w[c]) + m * mat_elems;
  gram<T, TILES>(x, p, K, si, sk, G, xs);
  __syncthreads();

  double off, trace;
  measure(G, p, &off, &trace);
  double lambda;
  if (!(fabs(trace) <= 1.79769313486231570815e308)) {
    lambda = trace;  // NaN or +inf: no sweeps
  } else {
    const int q = (p + 1) & ~1, half = q / 2;
    // (wave-uniform: off and trace are the butterfly's sums in every lane)
    for (int sweep = 0; sweep < kMaxSweeps && !(off <= 0x1p-104 * trace * trace); sweep++) {
      for (int round = 0; round < q - 1; round++) {
        if (lane < half) {
          Rot r;
          pair_of(round, lane, q, &r.a, &r.b);
          r.c = 1.0, r.s = 0.0, r.daa = 0.0, r.dbb = 0.0;
          if (r.b >= p) {
            r.a = -1;
          } else {
            const double aa = G[r.a * kLd + r.a], bb = G[r.b * kLd + r.b], ab = G[r.a * kLd + r.b];
            r.daa = aa, r.dbb = bb;
            if (ab != 0.0) {
              // t = tan of the angle that zeroes ab, the smaller root (|t| <= 1); a theta whose
              // square overflows gives t = 0 next to 1 / (2 theta), below the last bit of the diagonal
              const double theta = (bb - aa) / (2.0 * ab);
              const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
              r.c = 1.0 / sqrt(fma(t, t, 1.0)), r.s = t * r.c;
              r.daa = aa - t * ab, r.dbb = bb + t * ab;
            }
          }
          rot[lane] = r;
        }
        __syncthreads();
        // the columns: G <- G J
        for (int e = lane; e < half * p; e += kWave) {
          const int mm = e / p, k = e - mm * p;
          const Rot r = rot[mm];
          if (r.a < 0) continue;
          const double u = G[k * kLd + r.a], v = G[k * kLd + r.b];
          G[k * kLd + r.a] = r.c * u - r.s * v, G[k * kLd + r.b] = r.s * u + r.c * v;
        }
        __syncthreads();
        // the rows: G <- J^T G; the pair's own 2 x 2 block by the update formula
        for (int e = lane; e < half * p; e += kWave) {
          const int mm = e / p, k = e - mm * p;
          const Rot r = rot[mm];
          if (r.a < 0) continue;
          const double u = G[r.a * kLd + k], v = G[r.b * kLd + k];
          double nu = r.c * u - r.s * v, nv = r.s * u + r.c * v;
          if (k == r.a) nu = r.daa, nv = 0.0;
          if (k == r.b) nu = 0.0, nv = r.dbb;
          G[r.a * kLd + k] = nu, G[r.b * kLd + k] = nv;
        }
        __syncthreads();
      }
      measure(G, p, &off, &trace);
    }
    // the largest diagonal element; a NaN on the diagonal is the answer
    double best = lane < p ? G[lane * kLd + lane] : 0.0;
    bool nan = best != best;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double other = __shfl_xor(best, o, kWave);
      nan |= other != other;
      best = other > best ? other : best;
    }
    lambda = nan ? __builtin_nan("") : best;
  }
  if (lane == 0) {
    double sigma = sqrt(lambda > 0.0 || lambda != lambda ? lambda : 0.0);
    if (m < n_bn)
      sigma = sigma * bn_scale(reinterpret_cast<const T*>(px.bn_w[c]), reinterpret_cast<const T*>(px.bn_var[c]), m);
    out[c * n_mat + m] = sigma;
  }
}

// --- the BatchNorm features ---------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(wave::kBlock) k_bn(const Ptrs px, uint64_t n_bn, uint64_t total,
                                                     double* __restrict__ out) {
  for (uint64_t e = (uint64_t)blockIdx.x * wave::kBlock + threadIdx.x; e < total;
       e += (uint64_t)gridDim.x * wave::kBlock) {
    const uint64_t c = e / n_bn, ch = e - c * n_bn;
    out[e] = bn_scale(reinterpret_cast<const T*>(px.bn_w[c]), reinterpret_cast<const T*>(px.bn_var[c]), ch);
  }
}

// the table of one argument: required, element-aligned device pointers
static int take_table(const void* const* t, int n_clients, uintptr_t esz, const void** into, const char* what,
                      const char* name) {
  if (!t) {
    sa_set_error("%s: bad arguments (%s is required)", what, name);
    return SA_ERR_ARG;
  }
  for (int c = 0; c < n_clients; c++) {
    if (!t[c] || misaligned(t[c], esz)) {
      sa_set_error("%s: bad arguments (client %d's %s is required, element-aligned)", what, c, name);
      return SA_ERR_ARG;
    }
    into[c] = t[c];
  }
  return SA_OK;
}

static int check_clients(int n_clients, const char* what) {
  if (n_clients < 0 || n_clients > kMaxC) {
    sa_set_error("%s: n_clients must be in 0..%d (SA_FLAME_MAX_CLIENTS)", what, kMaxC);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

}  // namespace mars
}  // namespace sa

using namespace sa::mars;

extern "C" int sa_mars_sigma(const void* const* w, int n_clients, int x_type, uint64_t n_mat, uint64_t rows,
                             uint64_t cols, const void* const* bn_w, const void* const* bn_var, uint64_t n_bn,
                             double* out, void* stream) {
  const char* what = "sa_mars_sigma";
  int rc = check_float(x_type, what);
  if (rc == SA_OK) rc = check_clients(n_clients, what);
  // one block a matrix: the grid and every matrix's offset stay below 2^31 and 2^63
  if (rc == SA_OK) rc = check_n(n_mat, 24, what, " matrices (n_mat)");
  if (rc == SA_OK) rc = check_n(rows | cols, 24, what, " (rows, cols)");
  if (rc != SA_OK) return rc;
  const uint64_t p = rows < cols ? rows : cols, K = rows < cols ? cols : rows;
  if (p < 1 || p > (uint64_t)kMaxP) {
    sa_set_error("%s: min(rows, cols) must be in 1..%d (SA_MARS_MAX_P), got %llu", what, kMaxP,
                 (unsigned long long)p);
    return SA_ERR_UNSUPPORTED;
  }
  if (n_bn && (!bn_w || !bn_var)) {
    sa_set_error("%s: bad arguments (bn_w and bn_var are required with n_bn)", what);
    return SA_ERR_ARG;
  }
  if (n_clients == 0 || n_mat == 0) return SA_OK;
  if (!out || misaligned(out, 8)) {
    sa_set_error("%s: bad arguments (out is required, 8-byte aligned)", what);
    return SA_ERR_ARG;
  }
  const uintptr_t esz = elem_size(x_type);
  Ptrs px = {};
  rc = take_table(w, n_clients, esz, px.w, what, "w");
  if (rc == SA_OK && n_bn) rc = take_table(bn_w, n_clients, esz, px.bn_w, what, "bn_w");
  if (rc == SA_OK && n_bn) rc = take_table(bn_var, n_clients, esz, px.bn_var, what, "bn_var");
  if (rc != SA_OK) return rc;
  // X = W (rows < cols: K along the contiguous dimension) or W^T
  const uint64_t si = rows < cols ? cols : 1, sk = rows < cols ? 1 : cols;
  const dim3 grid((unsigned)(n_mat * (uint64_t)n_clients));
  hipStream_t st = (hipStream_t)stream;
  dispatch_float(x_type, [&](auto t) {
    typedef decltype(t) T;
    if (p <= 16)
      hipLaunchKernelGGL((k_sigma<T, 1>), grid, dim3(kWave), 0, st, px, n_mat, (int)p, K, si, sk, rows * cols, n_bn,
                         out);
    else
      hipLaunchKernelGGL((k_sigma<T, 2>), grid, dim3(kWave), 0, st, px, n_mat, (int)p, K, si, sk, rows * cols, n_bn,
                         out);
  });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_mars_bn(const void* const* bn_w, const void* const* bn_var, int n_clients, int x_type,
                          uint64_t n_bn, double* out, void* stream) {
  const char* what = "sa_mars_bn";
  int rc = check_float_n(x_type, n_bn, 32, what);
  if (rc == SA_OK) rc = check_clients(n_clients, what);
  if (rc != SA_OK) return rc;
  if (n_clients == 0 || n_bn == 0) return SA_OK;
  if (!out || misaligned(out, 8)) {
    sa_set_error("%s: bad arguments (out is required, 8-byte aligned)", what);
    return SA_ERR_ARG;
  }
  const uintptr_t esz = elem_size(x_type);
  Ptrs px = {};
  rc = take_table(bn_w, n_clients, esz, px.bn_w, what, "bn_w");
  if (rc == SA_OK) rc = take_table(bn_var, n_clients, esz, px.bn_var, what, "bn_var");
  if (rc != SA_OK) return rc;
  const uint64_t total = n_bn * (uint64_t)n_clients;
  uint64_t blocks = (total + sa::wave::kBlock - 1) / sa::wave::kBlock;
  if (blocks > (uint64_t)sa::wave::kMaxBlocks) blocks = sa::wave::kMaxBlocks;
  dispatch_float(x_type, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL((k_bn<T>), dim3((unsigned)blocks), dim3(sa::wave::kBlock), 0, (hipStream_t)stream, px, n_bn,
                       total, out);
  });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}
