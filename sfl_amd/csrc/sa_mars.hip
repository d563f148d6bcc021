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
//
// sigma of a wider layer (32 < p <= SA_MARS_WIDE_MAX_P; sa_mars_sigma_wide
// takes every p from 1): two kernels over a p x p float64 matrix a (client,
// matrix) in the caller's scratch.
//   k_gram_wide  G = X X^T.  A block of four waves (2 x 2) per 64 x 64 tile of
//      the upper triangle of G, a wave 2 x 2 accumulators of
//      v_mfma_f64_16x16x4_f64; k advances 16 a step through double-buffered
//      64 x 16 panels in LDS (sa_freq.hip's k_gemm: row stride 18 doubles, one
//      barrier a step).  Both panels come from X: a tile on the diagonal
//      stages and reads one, a tile off it stages two and is stored on both
//      sides of the diagonal; tiles below it have no block.  The staging
//      thread's (row, k) follows X's contiguous dimension.  No split along k.
//   k_eig_wide   one block of four waves a matrix, no grid-wide step:
//      1. the trace; not finite or not positive: sqrt(trace) is the value (NaN,
//         +inf or +0.0).  Else G is scaled in place by the power of two that
//         puts the trace in [1, 2): exact, and no square below can overflow.
//      2. Householder reduction to tridiagonal form in place, column by
//         column.  Column k's tail is read from row k (G is symmetric to the
//         bit, and stays so) into v (LDS); w = beta G v over the trailing
//         matrix with wave r on rows r, r + 4, ..., lane l on columns l,
//         l + 64, ... (eight accumulators a lane, every load coalesced along
//         a row), the waves' partial columns added in wave order through LDS;
//         w -= (beta / 2)(v . w) v; the trailing rank-2 update in the same
//         split.  Norms and dots: a thread's terms in index order, the wave's
//         butterfly, the waves in order.  A tail that is zero below the
//         subdiagonal takes no step.
//      3. diagonal and off-diagonal in LDS, the Gershgorin interval, and the
//         largest eigenvalue by Sturm counts in a multi-section: each of the
//         256 threads counts at one shift of the interval, the interval
//         becomes the gap around the first shift with every eigenvalue below
//         it; it ends when no shift lies strictly inside, and the upper end
//         is the eigenvalue.
//      4. scaled back, the square root, the BatchNorm scale: k_sigma's lines.
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

// --- wider layers: the Gram matrix in tiles --------------------------------------------
constexpr int kWideMaxP = SA_MARS_WIDE_MAX_P;
constexpr int kTile = 64;           // a block's tile of G: kTile x kTile
constexpr int kStep = 16;           // k a step
constexpr int kPanelLd = kStep + 2; // a panel's row stride in doubles (sa_freq.hip: 32-byte pieces tile the banks once)
constexpr int kPanel = kTile * kPanelLd;
constexpr double kTiny = 2.2250738585072014e-308;  // the smallest normal number

typedef double double2 __attribute__((ext_vector_type(2)));

// four doubles of a panel row: a row starts 16-byte aligned (kPanelLd is even), so two 16-byte accesses
__device__ __forceinline__ void put4(double* p, double4 v) {
  reinterpret_cast<double2*>(p)[0] = double2{v[0], v[1]};
  reinterpret_cast<double2*>(p)[1] = double2{v[2], v[3]};
}
__device__ __forceinline__ double4 get4(const double* p) {
  const double2 lo = reinterpret_cast<const double2*>(p)[0], hi = reinterpret_cast<const double2*>(p)[1];
  return double4{lo[0], lo[1], hi[0], hi[1]};
}

// X[row][k .. k + 3], zero outside p x K
template <class T>
__device__ __forceinline__ double4 fetch4(const T* __restrict__ x, uint64_t row, uint64_t k, int p, uint64_t K,
                                          uint64_t si, uint64_t sk) {
  double4 v = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < 4; s++) v[s] = x_at(x, row, k + s, p, K, si, sk);
  return v;
}

// grid (n_clients * n_mat, tiles (tiles + 1) / 2): blockIdx.y counts the tiles (ti, tj), tj >= ti, row by row.
// G of (client c, matrix m) = scratch + (c n_mat + m) p p, row-major, both triangles written.
template <class T>
__global__ void __launch_bounds__(wave::kBlock) k_gram_wide(const Ptrs px, uint64_t n_mat, int p, uint64_t K,
                                                            uint64_t si, uint64_t sk, uint64_t mat_elems, int tiles,
                                                            double* __restrict__ scratch) {
  __shared__ __attribute__((aligned(16))) double xs[2 * kPanel];
  __shared__ __attribute__((aligned(16))) double ys[2 * kPanel];
  const uint64_t cm = blockIdx.x, c = cm / n_mat, m = cm - c * n_mat;
  int ti = 0, rest = blockIdx.y;
  while (rest >= tiles - ti) rest -= tiles - ti, ti++;
  const bool diag = rest == 0;  // (block-uniform)
  const uint64_t i0 = (uint64_t)ti * kTile, j0 = (uint64_t)(ti + rest) * kTile;
  const T* x = reinterpret_cast<const T*>(px.w[c]) + m * mat_elems;
  double* G = scratch + cm * (uint64_t)p * (uint64_t)p;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int li = lane & 15, g = lane >> 4, wr = w >> 1, wc = w & 1;
  // staging: thread t moves four k of one row of either panel; consecutive threads along X's contiguous dimension
  const int srow = sk == 1 ? t >> 2 : t & 63, sk0 = (sk == 1 ? t & 3 : t >> 6) * 4;
  const double* bs = diag ? xs : ys;  // a diagonal tile's second operand is its first panel

  double4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++) acc[a][b] = double4{0.0, 0.0, 0.0, 0.0};

  double4 vx = fetch4(x, i0 + srow, (uint64_t)sk0, p, K, si, sk), vy = vx;
  if (!diag) vy = fetch4(x, j0 + srow, (uint64_t)sk0, p, K, si, sk);
  put4(&xs[srow * kPanelLd + sk0], vx);
  if (!diag) put4(&ys[srow * kPanelLd + sk0], vy);
  __syncthreads();
  const uint64_t steps = (K + kStep - 1) / kStep;
  for (uint64_t st = 0; st < steps; st++) {
    const int cur = (int)(st & 1) * kPanel, nxt = kPanel - cur;
    const bool more = st + 1 < steps;
    if (more) {
      vx = fetch4(x, i0 + srow, (st + 1) * kStep + sk0, p, K, si, sk);
      if (!diag) vy = fetch4(x, j0 + srow, (st + 1) * kStep + sk0, p, K, si, sk);
    }
    double4 a[2], b[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      a[h] = get4(&xs[cur + (32 * wr + 16 * h + li) * kPanelLd + 4 * g]);
      b[h] = get4(&bs[cur + (32 * wc + 16 * h + li) * kPanelLd + 4 * g]);
    }
#pragma unroll
    for (int s = 0; s < 4; s++)
#pragma unroll
      for (int ha = 0; ha < 2; ha++)
#pragma unroll
        for (int hb = 0; hb < 2; hb++)
          acc[ha][hb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ha][s], b[hb][s], acc[ha][hb], 0, 0, 0);
    if (more) {
      put4(&xs[nxt + srow * kPanelLd + sk0], vx);
      if (!diag) put4(&ys[nxt + srow * kPanelLd + sk0], vy);
    }
    __syncthreads();
  }
  // register r of lane group g: the 16 x 16 tile's element (4 r + g, li); G[i][j] and G[j][i] are the same
  // products in the same order of k, so a diagonal tile is symmetric to the bit without a mirrored store
#pragma unroll
  for (int ha = 0; ha < 2; ha++)
#pragma unroll
    for (int hb = 0; hb < 2; hb++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const uint64_t i = i0 + 32 * wr + 16 * ha + 4 * r + g, j = j0 + 32 * wc + 16 * hb + li;
        if (i < (uint64_t)p && j < (uint64_t)p) {
          G[i * p + j] = acc[ha][hb][r];
          if (!diag) G[j * p + i] = acc[ha][hb][r];
        }
      }
}

// --- wider layers: the largest eigenvalue -------------------------------------------------
// The block's reduction in a fixed order: the wave's butterfly, then the waves
// in order; every thread gets the result.  red: kWaves doubles of LDS.
template <class Op>
__device__ __forceinline__ double block_reduce(double v, double* red, Op op) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off, kWave));
  __syncthreads();  // the last call's readers are done with red
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return op(op(op(red[0], red[1]), red[2]), red[3]);
}
struct Add {
  __device__ __forceinline__ double operator()(double a, double b) const { return a + b; }
};
struct Min {
  __device__ __forceinline__ double operator()(double a, double b) const { return b < a ? b : a; }
};
struct Max {
  __device__ __forceinline__ double operator()(double a, double b) const { return b > a ? b : a; }
};

constexpr int kCols = kWideMaxP / kWave;  // a lane's columns of a trailing row
constexpr int kSections = wave::kBlock;   // shifts a round of the multi-section
constexpr int kMaxRounds = 80;            // far above what 2^-1074 of an interval takes; the loop ends before it

// how many eigenvalues of the tridiagonal matrix (d, e2 = e^2) lie below x
__device__ __forceinline__ int sturm(const double* d, const double* e2, int p, double x) {
  double q = d[0] - x;
  if (q == 0.0) q = kTiny;
  int below = q < 0.0;
  for (int i = 1; i < p; i++) {
    q = (d[i] - x) - e2[i - 1] / q;
    if (q == 0.0) q = kTiny;
    below += q < 0.0;
  }
  return below;
}

template <class T>
__global__ void __launch_bounds__(wave::kBlock) k_eig_wide(const Ptrs px, uint64_t n_mat, int p, uint64_t n_bn,
                                                           double* __restrict__ scratch, double* __restrict__ out) {
  __shared__ double v[kWideMaxP], w[kWideMaxP], d[kWideMaxP], e[kWideMaxP];
  __shared__ double part[wave::kWaves * kWideMaxP];  // the waves' partial columns; then the round's shifts
  __shared__ int full[kSections];
  __shared__ double red[wave::kWaves];
  const uint64_t cm = blockIdx.x, c = cm / n_mat, m = cm - c * n_mat;
  double* G = scratch + cm * (uint64_t)p * (uint64_t)p;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;

  double tr = 0.0;
  for (int i = t; i < p; i += wave::kBlock) tr += G[(uint64_t)i * p + i];
  const double trace = block_reduce(tr, red, Add());
  double lambda = trace;  // NaN, +inf, or nothing to find: k_sigma's rule
  if (trace > 0.0 && trace <= 1.79769313486231570815e308) {  // (block-uniform: every thread has the same sum)
    const int ex = ilogb(trace);
    for (int idx = t; idx < p * p; idx += wave::kBlock) G[idx] = ldexp(G[idx], -ex);
    __syncthreads();

    // --- Householder: column k's tail x = G[k][k + 1 ..] becomes (alpha, 0, ...) ---
    for (int k = 0; k + 2 < p; k++) {
      const int L = p - k - 1;  // the trailing matrix: L x L from (k + 1, k + 1)
      double* A = G + (uint64_t)(k + 1) * p + (k + 1);
      double s2 = 0.0;
      for (int j = t; j < L; j += wave::kBlock) {
        const double xj = G[(uint64_t)k * p + k + 1 + j];
        v[j] = xj;
        if (j) s2 += xj * xj;
      }
      s2 = block_reduce(s2, red, Add());
      const double x0 = v[0];
      if (s2 < kTiny) {  // nothing below the subdiagonal (block-uniform): no step
        if (t == 0) d[k] = G[(uint64_t)k * p + k], e[k] = x0;
      } else {
        const double norm = sqrt(x0 * x0 + s2), alpha = x0 >= 0.0 ? -norm : norm, v0 = x0 - alpha;
        const double beta = 2.0 / (v0 * v0 + s2);
        __syncthreads();  // every thread has read x0
        if (t == 0) v[0] = v0, d[k] = G[(uint64_t)k * p + k], e[k] = alpha;
        __syncthreads();
        // w = beta A v: wave wv's rows, lane's columns; A is symmetric, so a column's sum over rows is a row's
        double acc[kCols], vj[kCols], wj[kCols];
#pragma unroll
        for (int cc = 0; cc < kCols; cc++) acc[cc] = 0.0;
        for (int i = wv; i < L; i += wave::kWaves) {
          const double vi = v[i];
          const double* row = A + (uint64_t)i * p;
#pragma unroll
          for (int cc = 0; cc < kCols; cc++) {
            const int j = lane + kWave * cc;
            if (j < L) acc[cc] += row[j] * vi;
          }
        }
#pragma unroll
        for (int cc = 0; cc < kCols; cc++) {
          const int j = lane + kWave * cc;
          if (j < L) part[wv * kWideMaxP + j] = acc[cc];
        }
        __syncthreads();
        double dot = 0.0;
        for (int j = t; j < L; j += wave::kBlock) {
          const double wj0 = beta * (((part[j] + part[kWideMaxP + j]) + part[2 * kWideMaxP + j]) + part[3 * kWideMaxP + j]);
          w[j] = wj0;
          dot += v[j] * wj0;
        }
        dot = block_reduce(dot, red, Add());
        const double half = 0.5 * beta * dot;
        for (int j = t; j < L; j += wave::kBlock) w[j] = w[j] - half * v[j];
        __syncthreads();
        // A -= v w^T + w v^T: (i, j) and (j, i) get the same two products, added in either order
#pragma unroll
        for (int cc = 0; cc < kCols; cc++) {
          const int j = lane + kWave * cc;
          vj[cc] = j < L ? v[j] : 0.0, wj[cc] = j < L ? w[j] : 0.0;
        }
        for (int i = wv; i < L; i += wave::kWaves) {
          const double vi = v[i], wi = w[i];
          double* row = A + (uint64_t)i * p;
#pragma unroll
          for (int cc = 0; cc < kCols; cc++) {
            const int j = lane + kWave * cc;
            if (j < L) row[j] = row[j] - (vi * wj[cc] + wi * vj[cc]);
          }
        }
      }
      __syncthreads();  // the trailing matrix and v, w before the next column
    }
    if (t == 0) {
      d[p - 1] = G[(uint64_t)(p - 1) * p + p - 1];
      if (p > 1) d[p - 2] = G[(uint64_t)(p - 2) * p + p - 2], e[p - 2] = G[(uint64_t)(p - 2) * p + p - 1];
    }
    __syncthreads();

    // --- the Gershgorin interval, e^2 into w ---
    double lo = 1.79769313486231570815e308, hi = -lo;
    for (int i = t; i < p; i += wave::kBlock) {
      const double r = (i ? fabs(e[i - 1]) : 0.0) + (i + 1 < p ? fabs(e[i]) : 0.0);
      lo = Min()(lo, d[i] - r), hi = Max()(hi, d[i] + r);
      if (i + 1 < p) w[i] = e[i] * e[i];
    }
    lo = block_reduce(lo, red, Min());
    hi = block_reduce(hi, red, Max());  // (its barriers publish w)

    // --- the multi-section: the upper end keeps every eigenvalue at or below it ---
    double* shift = part;
    for (int round = 0; round < kMaxRounds; round++) {
      const double xt = lo + (hi - lo) * (1.0 / (kSections + 1)) * (double)(t + 1);
      const bool inside = lo < xt && xt < hi;
      shift[t] = xt;
      full[t] = inside ? (sturm(d, w, p, xt) == p ? 2 : 1) : 0;  // 0: no shift of its own
      __syncthreads();
      // every thread walks the shifts in order: the last one below the top eigenvalue, the first one above
      double nlo = lo, nhi = hi;
      bool any = false;
      for (int s = 0; s < kSections; s++) {
        const int f = full[s];
        const double xs = shift[s];
        any |= f != 0;
        if (f == 1 && xs > nlo && xs < nhi) nlo = xs;
        if (f == 2 && xs < nhi) nhi = xs;
      }
      lo = nlo, hi = nhi;  // (the shifts ascend with s, so nlo < nhi whatever the counts say)
      __syncthreads();  // the shifts are read before the next round's
      if (!any) break;  // (block-uniform) the interval cannot be split further
    }
    lambda = ldexp(hi, ex);
  }
  if (t == 0) {
    double sigma = sqrt(lambda > 0.0 || lambda != lambda ? lambda : 0.0);
    if (m < n_bn)
      sigma = sigma * bn_scale(reinterpret_cast<const T*>(px.bn_w[c]), reinterpret_cast<const T*>(px.bn_var[c]), m);
    out[cm] = sigma;
  }
}

// the scalars of a wide call; *bytes gets the scratch's size
static int check_wide(int n_clients, uint64_t n_mat, uint64_t rows, uint64_t cols, const char* what, uint64_t* bytes) {
  int rc = check_clients(n_clients, 0, kMaxC, what);
  if (rc == SA_OK) rc = check_n(n_mat, 24, what, " matrices (n_mat)");
  if (rc == SA_OK) rc = check_n(rows | cols, 24, what, " (rows, cols)");
  if (rc != SA_OK) return rc;
  const uint64_t p = rows < cols ? rows : cols;
  if (p < 1 || p > (uint64_t)kWideMaxP) {
    sa_set_error("%s: min(rows, cols) must be in 1..%d (SA_MARS_WIDE_MAX_P), got %llu", what, kWideMaxP,
                 (unsigned long long)p);
    return SA_ERR_UNSUPPORTED;
  }
  *bytes = (uint64_t)n_clients * n_mat * p * p * 8;  // (below 2^4 * 2^24 * 2^18 * 2^3)
  if (*bytes > 0x7fffffffull) {
    sa_set_error("%s: %d clients of %llu matrices with a smaller side of %llu need %llu bytes of scratch, above "
                 "2^31 - 1", what, n_clients, (unsigned long long)n_mat, (unsigned long long)p,
                 (unsigned long long)*bytes);
    return SA_ERR_UNSUPPORTED;
  }
  return SA_OK;
}

}  // namespace mars
}  // namespace sa

using namespace sa::mars;

extern "C" int sa_mars_wide_scratch_bytes(int n_clients, uint64_t n_mat, uint64_t rows, uint64_t cols) {
  uint64_t bytes = 0;
  const int rc = check_wide(n_clients, n_mat, rows, cols, "sa_mars_wide_scratch_bytes", &bytes);
  return rc != SA_OK ? rc : (int)bytes;
}

extern "C" int sa_mars_sigma_wide(const void* const* w, int n_clients, int x_type, uint64_t n_mat, uint64_t rows,
                                  uint64_t cols, const void* const* bn_w, const void* const* bn_var, uint64_t n_bn,
                                  void* scratch, double* out, void* stream) {
  const char* what = "sa_mars_sigma_wide";
  uint64_t bytes = 0;
  int rc = check_float(x_type, what);
  if (rc == SA_OK) rc = check_wide(n_clients, n_mat, rows, cols, what, &bytes);
  if (rc != SA_OK) return rc;
  if (n_bn && (!bn_w || !bn_var)) {
    sa_set_error("%s: bad arguments (bn_w and bn_var are required with n_bn)", what);
    return SA_ERR_ARG;
  }
  if (n_clients == 0 || n_mat == 0) return SA_OK;
  if (!out || misaligned(out, 8) || !scratch || misaligned(scratch, 8)) {
    sa_set_error("%s: bad arguments (scratch and out are required, 8-byte aligned)", what);
    return SA_ERR_ARG;
  }
  const uintptr_t esz = elem_size(x_type);
  Ptrs px = {};
  rc = take_table(w, n_clients, esz, px.w, what, "w");
  if (rc == SA_OK && n_bn) rc = take_table(bn_w, n_clients, esz, px.bn_w, what, "bn_w");
  if (rc == SA_OK && n_bn) rc = take_table(bn_var, n_clients, esz, px.bn_var, what, "bn_var");
  if (rc != SA_OK) return rc;
  const uint64_t p = rows < cols ? rows : cols, K = rows < cols ? cols : rows;
  const uint64_t si = rows < cols ? cols : 1, sk = rows < cols ? 1 : cols;
  const int tiles = (int)((p + kTile - 1) / kTile);
  // (the scratch's bound keeps n_mat * n_clients below 2^28)
  const unsigned mats = (unsigned)(n_mat * (uint64_t)n_clients);
  hipStream_t st = (hipStream_t)stream;
  dispatch_float(x_type, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL((k_gram_wide<T>), dim3(mats, (unsigned)(tiles * (tiles + 1) / 2)), dim3(sa::wave::kBlock), 0, st,
                       px, n_mat, (int)p, K, si, sk, rows * cols, tiles, reinterpret_cast<double*>(scratch));
    hipLaunchKernelGGL((k_eig_wide<T>), dim3(mats), dim3(sa::wave::kBlock), 0, st, px, n_mat, (int)p, n_bn,
                       reinterpret_cast<double*>(scratch), out);
  });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_mars_sigma(const void* const* w, int n_clients, int x_type, uint64_t n_mat, uint64_t rows,
                             uint64_t cols, const void* const* bn_w, const void* const* bn_var, uint64_t n_bn,
                             double* out, void* stream) {
  const char* what = "sa_mars_sigma";
  int rc = check_float(x_type, what);
  if (rc == SA_OK) rc = check_clients(n_clients, 0, kMaxC, what);
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
  if (rc == SA_OK) rc = check_clients(n_clients, 0, kMaxC, what);
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
