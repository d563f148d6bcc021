// sa_freq.hip — the feature extraction of FreqAggregator on the device (the
// reference's FreqFed robust aggregator, examples/security/h_bd/
// agg_freqfed.py:26-61 and :80-87; sfl_amd/security/aggregation/
// freq_aggregator.py has the definition and the host form, DESIGN.md §23 the
// split and the LDS use):
//
//   F_c  = the low-frequency corner (hk x wk) of the orthonormal 2-D DCT-II of
//          client c's rows x cols matrix W_c, in float64:
//          F_c = A W_c B^T with A = C_rows[:hk], B = C_cols[:wk], entries with
//          i + j > q stored as +0.0
//   G    = the packed upper triangle of the clients' Gram matrix F_i . F_j
//
// Three kernels.  k_basis writes A and B into scratch; every argument of a
// cosine is reduced exactly in integers first.  k_gemm is both products:
// D[i][j] = sum_k X[i][k] Y[j][k] with X a float64 matrix all clients share
// (B, then A) and Y one matrix a client (W_c in the upload's type, then the
// first product).  The first product is formed transposed, Tt_c = B W_c^T
// (wk x rows), so that it is stored along its rows and read along k by the
// second, F_c = A Tt_c^T: neither product stores against the grain.
//
// k_gemm: a block of four waves (2 x 2) owns a 64 x 64 tile of D, a wave a
// 32 x 32 piece as 2 x 2 accumulators of v_mfma_f64_16x16x4_f64 (16 doubles a
// lane).  k advances 16 a step through double-buffered 64 x 16 panels of X and
// Y in LDS (row stride 18 doubles: the 16 lanes of a lane group read their four
// consecutive k as 32-byte pieces that tile the 64 banks once), float32
// converted as it is staged, rows and k outside the matrices staged as zero;
// one barrier a step.  Operands as in sa_mars.hip: lane l holds X[l % 16][k]
// and Y[l % 16][k] for k = 4 (l / 16) + s, MFMA s = 0..3 of a step; result
// register r of lane group g is D[4 r + g][l % 16].  No split along k, no
// atomics: the order of every sum is a function of the shapes and the same
// input gives the same bits.  A tile of the second product that lies wholly
// behind the filter's diagonal is stored as zeros without a product.
//
// k_gram: one block a pair (i <= j); a lane's partial sum in index order, the
// wave's butterfly, the four waves in order.
#include <hip/hip_runtime.h>

#include "sa_compress.h"

namespace sa {
namespace freq {

using namespace sa::entry;

constexpr int kMaxC = SA_FLAME_MAX_CLIENTS;
constexpr int kTile = 64;         // a block's tile of D: kTile x kTile
constexpr int kStep = 16;         // k a step
constexpr int kLd = kStep + 2;    // a panel's row stride in doubles
constexpr int kPanel = kTile * kLd;
constexpr uint32_t kNoFilter = 0xffffffffu;

typedef double double4 __attribute__((ext_vector_type(4)));
typedef double double2 __attribute__((ext_vector_type(2)));

// four doubles of a panel row: a row starts 16-byte aligned (kLd is even), so two 16-byte accesses
__device__ __forceinline__ void put4(double* p, double4 v) {
  reinterpret_cast<double2*>(p)[0] = double2{v[0], v[1]};
  reinterpret_cast<double2*>(p)[1] = double2{v[2], v[3]};
}
__device__ __forceinline__ double4 get4(const double* p) {
  const double2 lo = reinterpret_cast<const double2*>(p)[0], hi = reinterpret_cast<const double2*>(p)[1];
  return double4{lo[0], lo[1], hi[0], hi[1]};
}

// the per-client operand's pointers, by value: no device allocation holds the table
struct Ptrs {
  const void* y[kMaxC];
};

// the corner of a rows x cols matrix (freq_aggregator.py, step 3)
struct Corner {
  uint64_t hk, wk, q;
};
inline Corner corner(uint64_t rows, uint64_t cols) {
  Corner c;
  c.q = (rows + cols) / 4;
  c.hk = rows / 2 < c.q + 1 ? rows / 2 : c.q + 1;
  c.wk = cols / 2 < c.q + 1 ? cols / 2 : c.q + 1;
  return c;
}

// --- the basis ------------------------------------------------------------------
// C_n[k][i] = s_k cos(pi (2 i + 1) k / (2 n)): r = (2 i + 1) k mod 4 n is the
// angle in units of pi / (2 n); folded into the first quadrant, so that
// entries that are equal in magnitude get equal bits and a quarter period is +0.0
__device__ __forceinline__ double basis_at(uint64_t k, uint64_t i, uint64_t n) {
  uint64_t r = ((2 * i + 1) * k) % (4 * n);
  if (r > 2 * n) r = 4 * n - r;  // cos(2 pi - x) = cos(x)
  const bool neg = r > n;
  if (neg) r = 2 * n - r;  // cos(pi - x) = -cos(x)
  if (r == n) return 0.0;
  const double c = cospi((double)r / (double)(2 * n)) * sqrt((k == 0 ? 1.0 : 2.0) / (double)n);
  return neg ? -c : c;
}

__global__ void __launch_bounds__(wave::kBlock) k_basis(double* __restrict__ A, uint64_t hk, uint64_t rows,
                                                        double* __restrict__ B, uint64_t wk, uint64_t cols) {
  const uint64_t na = hk * rows, total = na + wk * cols;
  for (uint64_t e = (uint64_t)blockIdx.x * wave::kBlock + threadIdx.x; e < total;
       e += (uint64_t)gridDim.x * wave::kBlock) {
    if (e < na) A[e] = basis_at(e / rows, e % rows, rows);
    else B[e - na] = basis_at((e - na) / cols, (e - na) % cols, cols);
  }
}

// --- the products -----------------------------------------------------------------
// four consecutive k of one row of a panel, zero outside rows x K
template <class T>
__device__ __forceinline__ double4 fetch(const T* __restrict__ m, uint64_t row, uint64_t rows, uint64_t k, uint64_t K) {
  double4 v = {0.0, 0.0, 0.0, 0.0};
  if (row < rows) {
    const T* p = m + row * K;
#pragma unroll
    for (int s = 0; s < 4; s++)
      if (k + s < K) v[s] = (double)p[k + s];
  }
  return v;
}

// D[i][j] = sum_k X[i][k] Y_c[j][k], i < I, j < J, k < K; D_c = out + c * I * J, row-major;
// entries with i + j > q are stored as +0.0 (q = kNoFilter: none are)
template <class T>
__global__ void __launch_bounds__(wave::kBlock) k_gemm(const double* __restrict__ X, const Ptrs py, uint64_t I,
                                                       uint64_t J, uint64_t K, uint32_t tiles_j, uint32_t q,
                                                       double* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) double xs[2 * kPanel];
  __shared__ __attribute__((aligned(16))) double ys[2 * kPanel];
  const uint64_t i0 = (uint64_t)(blockIdx.x / tiles_j) * kTile, j0 = (uint64_t)(blockIdx.x % tiles_j) * kTile;
  const T* Y = reinterpret_cast<const T*>(py.y[blockIdx.y]);
  double* D = out + (uint64_t)blockIdx.y * I * J;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int li = lane & 15, g = lane >> 4, wr = w >> 1, wc = w & 1;

  double4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++) acc[a][b] = double4{0.0, 0.0, 0.0, 0.0};

  if (i0 + j0 <= (uint64_t)q) {  // (block-uniform) else: the whole tile is behind the diagonal
    // staging: thread t moves four consecutive k of row t / 4 of either panel
    const int srow = t >> 2, sk = (t & 3) * 4;
    double4 vx = fetch(X, i0 + srow, I, (uint64_t)sk, K), vy = fetch(Y, j0 + srow, J, (uint64_t)sk, K);
    put4(&xs[srow * kLd + sk], vx);
    put4(&ys[srow * kLd + sk], vy);
    __syncthreads();
    const uint64_t steps = (K + kStep - 1) / kStep;
    for (uint64_t st = 0; st < steps; st++) {
      const int cur = (int)(st & 1) * kPanel, nxt = kPanel - cur;
      const bool more = st + 1 < steps;
      if (more) {
        vx = fetch(X, i0 + srow, I, (st + 1) * kStep + sk, K);
        vy = fetch(Y, j0 + srow, J, (st + 1) * kStep + sk, K);
      }
      double4 a[2], b[2];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        a[h] = get4(&xs[cur + (32 * wr + 16 * h + li) * kLd + 4 * g]);
        b[h] = get4(&ys[cur + (32 * wc + 16 * h + li) * kLd + 4 * g]);
      }
#pragma unroll
      for (int s = 0; s < 4; s++)
#pragma unroll
        for (int ha = 0; ha < 2; ha++)
#pragma unroll
          for (int hb = 0; hb < 2; hb++)
            acc[ha][hb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ha][s], b[hb][s], acc[ha][hb], 0, 0, 0);
      if (more) {
        put4(&xs[nxt + srow * kLd + sk], vx);
        put4(&ys[nxt + srow * kLd + sk], vy);
      }
      __syncthreads();
    }
  }
  // register r of lane group g: the 16 x 16 tile's element (4 r + g, li)
#pragma unroll
  for (int ha = 0; ha < 2; ha++)
#pragma unroll
    for (int hb = 0; hb < 2; hb++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const uint64_t i = i0 + 32 * wr + 16 * ha + 4 * r + g, j = j0 + 32 * wc + 16 * hb + li;
        if (i < I && j < J) D[i * J + j] = i + j > (uint64_t)q ? 0.0 : acc[ha][hb][r];
      }
}

// --- the Gram matrix ----------------------------------------------------------------
__global__ void __launch_bounds__(wave::kBlock) k_gram(const double* __restrict__ feats, int n_clients, uint64_t len,
                                                       double* __restrict__ out) {
  __shared__ double part[wave::kWaves];
  // pair blockIdx.x of the upper triangle, row-major: (i, j), j >= i
  int i = 0, rest = blockIdx.x;
  while (rest >= n_clients - i) rest -= n_clients - i, i++;
  const double* a = feats + (uint64_t)i * len;
  const double* b = feats + (uint64_t)(i + rest) * len;
  double s = 0.0;
#pragma unroll 4
  for (uint64_t e = threadIdx.x; e < len; e += wave::kBlock) s = fma(a[e], b[e], s);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

// --- the entries' checks ----------------------------------------------------------------
// the scalars of a features call; *bytes gets the scratch's size
static int check_shape(uint64_t rows, uint64_t cols, int n_clients, int x_type, const char* what, uint64_t* bytes) {
  int rc = check_float(x_type, what);
  if (rc == SA_OK) rc = check_clients(n_clients, 0, kMaxC, what);
  if (rc == SA_OK) rc = check_n(rows | cols, 24, what, " (rows, cols)");
  if (rc != SA_OK) return rc;
  if (rows < 2 || cols < 2) {
    sa_set_error("%s: rows and cols must be at least 2 (a smaller matrix has no corner)", what);
    return SA_ERR_ARG;
  }
  const Corner c = corner(rows, cols);
  // A, B, and every client's first product (all below 2^24 * 2^24 * 2^5)
  *bytes = 8 * (c.hk * rows + c.wk * cols + (uint64_t)n_clients * c.wk * rows);
  const uint64_t tiles = ((c.wk + kTile - 1) / kTile) * ((rows + kTile - 1) / kTile);
  if (*bytes > 0x7fffffffull || tiles > 0x7fffffffull) {
    sa_set_error("%s: a %llu x %llu corner of %d clients needs %llu bytes of scratch, above 2^31 - 1", what,
                 (unsigned long long)c.hk, (unsigned long long)c.wk, n_clients, (unsigned long long)*bytes);
    return SA_ERR_UNSUPPORTED;
  }
  return SA_OK;
}

}  // namespace freq
}  // namespace sa

using namespace sa::freq;

extern "C" int sa_freq_scratch_bytes(uint64_t rows, uint64_t cols, int n_clients, int x_type) {
  uint64_t bytes = 0;
  const int rc = check_shape(rows, cols, n_clients, x_type, "sa_freq_scratch_bytes", &bytes);
  return rc != SA_OK ? rc : (int)bytes;
}

extern "C" int sa_freq_features(const void* const* w, int n_clients, int x_type, uint64_t rows, uint64_t cols,
                                void* scratch, double* feats_out, void* stream) {
  const char* what = "sa_freq_features";
  uint64_t bytes = 0;
  int rc = check_shape(rows, cols, n_clients, x_type, what, &bytes);
  if (rc != SA_OK) return rc;
  if (n_clients == 0) return SA_OK;
  if (!w || !scratch || !feats_out || misaligned(scratch, 8) || misaligned(feats_out, 8)) {
    sa_set_error("%s: bad arguments (w, scratch and feats_out are required; 8-byte aligned scratch and feats_out)",
                 what);
    return SA_ERR_ARG;
  }
  const uintptr_t esz = elem_size(x_type);
  Ptrs pw = {}, pt = {};
  const Corner c = corner(rows, cols);
  double* A = reinterpret_cast<double*>(scratch);
  double* B = A + c.hk * rows;
  double* Tt = B + c.wk * cols;
  rc = take_table(w, n_clients, esz, pw.y, what, "w");  // (w is there: the check above)
  if (rc != SA_OK) return rc;
  for (int i = 0; i < n_clients; i++) pt.y[i] = Tt + (uint64_t)i * c.wk * rows;
  hipStream_t st = (hipStream_t)stream;
  uint64_t blocks = (c.hk * rows + c.wk * cols + sa::wave::kBlock - 1) / sa::wave::kBlock;
  if (blocks > (uint64_t)sa::wave::kMaxBlocks) blocks = sa::wave::kMaxBlocks;
  hipLaunchKernelGGL(k_basis, dim3((unsigned)blocks), dim3(sa::wave::kBlock), 0, st, A, c.hk, rows, B, c.wk, cols);
  // Tt_c = B W_c^T: wk x rows over k < cols
  const uint32_t tj1 = (uint32_t)((rows + kTile - 1) / kTile), ti1 = (uint32_t)((c.wk + kTile - 1) / kTile);
  dispatch_float(x_type, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL((k_gemm<T>), dim3(ti1 * tj1, (unsigned)n_clients), dim3(sa::wave::kBlock), 0, st, B, pw, c.wk,
                       rows, cols, tj1, kNoFilter, Tt);
  });
  // F_c = A Tt_c^T: hk x wk over k < rows, the filter applied
  const uint32_t tj2 = (uint32_t)((c.wk + kTile - 1) / kTile), ti2 = (uint32_t)((c.hk + kTile - 1) / kTile);
  hipLaunchKernelGGL((k_gemm<double>), dim3(ti2 * tj2, (unsigned)n_clients), dim3(sa::wave::kBlock), 0, st, A, pt, c.hk,
                     c.wk, rows, tj2, (uint32_t)c.q, feats_out);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_freq_gram(const double* feats, int n_clients, uint64_t len, double* out, void* stream) {
  const char* what = "sa_freq_gram";
  int rc = check_n(len, 32, what);
  if (rc == SA_OK) rc = check_clients(n_clients, 0, kMaxC, what);
  if (rc != SA_OK) return rc;
  if (n_clients == 0) return SA_OK;
  if (!feats || !out || misaligned(feats, 8) || misaligned(out, 8)) {
    sa_set_error("%s: bad arguments (feats and out are required, 8-byte aligned)", what);
    return SA_ERR_ARG;
  }
  hipLaunchKernelGGL(k_gram, dim3((unsigned)(n_clients * (n_clients + 1) / 2)), dim3(sa::wave::kBlock), 0,
                     (hipStream_t)stream, feats, n_clients, len, out);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}
