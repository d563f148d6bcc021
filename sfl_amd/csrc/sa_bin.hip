// sa_bin.hip — HomoBinning's local quantities on the device: what one party
// computes from its rows x F data for the reference's federated quantile
// binning (sfl/preprocessing/binning/homo_binning_base.py:150-159 and
// :208-247; sfl_amd/preprocessing/binning/homo_binning.py has the definition
// and the host form).  Two passes over x, both exact and both integer- or
// order-free, so a device party gives the bits of a host party:
//
//   range   per feature min, max (float64), count of valid values and of
//           NaN; once per fit
//   ranks   per feature and query point q the number of valid x < q; once
//           per round of the bisection, the hot path
//
// The work split (both passes).  x is row-major.  A block column (blockIdx.y)
// owns a group of fg <= 64 neighbouring columns, w of them in the last group.
// A wave covers floor(64 / w) whole rows of the group per step: lane l holds
// row l / w of the step and column l % w of the group, for the kernel's life.
// Where the group is the whole row (F <= 64) the wave's elements of a step are
// one contiguous run of memory; otherwise one run of w elements per row.  A
// lane's feature never changes, so what belongs to the feature (its query
// points, its counters, its extrema) lives in the lane's registers.  The four
// waves of a block interleave their steps over the block's rows [lo, hi), and
// a wave keeps kUnroll loads in flight.
//
// ranks, register form (Q <= 16): the lane holds its feature's Q query points
// and Q 32-bit counters; an element costs one validity test and Q compare /
// add-with-carry pairs, no search, no LDS, no atomics.  At the end the lanes
// of one feature are summed with shuffles, the block's waves through LDS, and
// the block adds Q 64-bit integers a feature into the output.
// ranks, LDS form (17 <= Q <= 255): the group's tables sit in LDS, padded to
// a power of two with NaN; an element is one branch-free binary search for
// c = #{q_j <= x} and one LDS integer add into [feature][c]; x < q_j holds
// exactly when c <= j, so an inclusive scan over c at the end gives the ranks.
//
// float32 data compare against float32 query points: up32(q), the smallest
// float32 >= q, staged once per block.  For a float32 x, x < q holds exactly
// when x < up32(q): if x < q then x < q <= up32(q); if x >= q then x is a
// float32 that is >= q, so x >= up32(q), the smallest such.  A q above FLT_MAX
// becomes +inf, a NaN stays NaN (the pad: it counts nothing).
#include <hip/hip_runtime.h>

#include "sa_compress.h"

namespace sa {
namespace bin {

using namespace sa::entry;
using namespace sa::wave;

constexpr int kRegMaxQ = SA_BIN_REG_MAX_Q;
constexpr int kMaxQ = SA_BIN_MAX_Q;
constexpr int kMaxAbnormal = SA_BIN_MAX_ABNORMAL;
constexpr int kUnroll = 8;           // loads a wave keeps in flight
constexpr int kLdsBudget = 65536;    // sa_hist.hip's: two blocks resident, no opt-in
constexpr int kMaxTiles = 1024;      // blocks of a launch over all groups, as sa_hist.hip's build
constexpr uint64_t kMaxLen = 1ull << 31;  // rows of a block: no 32-bit counter wraps

// --- geometry (host) ----------------------------------------------------------

struct Geometry {
  int form;    // 0: registers, 1: LDS
  int qp;      // query points per feature, padded: 4, 8 or 16; or the power of two above Q
  int fg;      // columns per group
  int lds;     // bytes of LDS of a block
  int groups;  // gridDim.y
};

// Q in 1..255, F >= 1, esz 4 or 8
inline Geometry bin_geometry(int Q, uint64_t F, int esz) {
  Geometry g;
  int cap = 64;
  if (Q <= kRegMaxQ) {
    g.form = 0, g.qp = Q <= 4 ? 4 : Q <= 8 ? 8 : 16;
    g.lds = 64 * g.qp * 4;  // the block's counters
  } else {
    g.form = 1, g.qp = 32;
    while (g.qp <= Q) g.qp <<= 1;  // qp - 1 >= Q entries are searched
    const int fit = kLdsBudget / (g.qp * (esz + 4));  // a table entry and a counter
    if (fit < cap) cap = fit;                         // >= 21: 256 x 12 bytes a feature
  }
  g.fg = F < (uint64_t)cap ? (int)F : cap;
  if (g.form) g.lds = g.fg * g.qp * (esz + 4);
  g.groups = (int)((F + g.fg - 1) / g.fg);
  return g;
}

struct Rows {
  uint64_t tiles, len;  // gridDim.x, rows per block
};
// the row split of a launch whose full groups have fg columns
inline Rows rows_grid(uint64_t rows, int fg, int groups) {
  const uint64_t per_step = (uint64_t)(64 / fg) * kWaves * kUnroll;
  uint64_t tiles = (rows + per_step - 1) / per_step;
  const uint64_t cap = kMaxTiles / groups ? kMaxTiles / groups : 1;
  if (tiles > cap) tiles = cap;
  const uint64_t least = (rows + kMaxLen - 1) / kMaxLen;
  if (tiles < least) tiles = least;
  if (tiles == 0) tiles = 1;
  Rows r;
  r.len = (rows + tiles - 1) / tiles;
  if (r.len == 0) r.len = 1;
  r.tiles = rows ? (rows + r.len - 1) / r.len : 1;
  return r;
}

// --- the lane layout ------------------------------------------------------------

struct Abnormal {
  double v[kMaxAbnormal];  // NaN beyond n
  int n;
};

template <class T>
struct Sieve {
  T a[kMaxAbnormal];
  int n;
  __device__ __forceinline__ explicit Sieve(const Abnormal& ab) : n(ab.n) {
#pragma unroll
    for (int i = 0; i < kMaxAbnormal; i++) a[i] = (T)ab.v[i];  // the data's dtype: numpy's float32(a)
  }
  // v, or NaN for an abnormal value (n is uniform: a scalar branch)
  __device__ __forceinline__ T operator()(T v) const {
    if (n) {
      const bool bad = v == a[0] || v == a[1] || v == a[2] || v == a[3];
      v = bad ? (T)__builtin_nan("") : v;
    }
    return v;
  }
};

struct Lane {
  uint64_t f0;  // the group's first column
  int w;        // the group's columns
  int col;      // this lane's column in the group
  int row;      // this lane's row in a step
  int rps;      // rows per step of a wave
  bool active;
};
__device__ __forceinline__ Lane lane_of(uint64_t F, int fg) {
  Lane l;
  l.f0 = (uint64_t)blockIdx.y * fg;
  l.w = F - l.f0 < (uint64_t)fg ? (int)(F - l.f0) : fg;
  l.rps = 64 / l.w;
  const int lane = threadIdx.x & 63;
  l.row = lane / l.w;
  l.col = lane - l.row * l.w;
  l.active = l.row < l.rps;
  return l;
}

// The lane's elements of kUnroll steps from row base rb on; NaN where the lane
// is idle or the row is at or beyond hi.  px = x + f0 + col.  ok: bit u set
// where v[u] was read.
template <class T>
__device__ __forceinline__ uint32_t load_steps(const T* px, uint64_t F, uint64_t rb, uint64_t hi, const Lane& l,
                                               T (&v)[kUnroll]) {
  const uint64_t step = (uint64_t)kWaves * l.rps;
  uint32_t ok = 0;
#pragma unroll
  for (int u = 0; u < kUnroll; u++) {
    const uint64_t r = rb + u * step + l.row;
    const bool in = l.active && r < hi;
    v[u] = in ? px[r * F] : (T)__builtin_nan("");
    ok |= in ? 1u << u : 0u;
  }
  return ok;
}

// the sum over the lanes of one column (row 0's lane ends with it): a tree over
// the rows of a step; a lane beyond the wave adds nothing
__device__ __forceinline__ uint32_t column_sum(uint32_t c, const Lane& l) {
  const int lane = threadIdx.x & 63;
  for (int s = 1; s < l.rps; s <<= 1) {
    const uint32_t u = (uint32_t)__shfl_down((int)c, s * l.w, 64);
    if (lane + s * l.w < 64) c += u;
  }
  return c;
}

// --- staging the query points -------------------------------------------------------

__device__ __forceinline__ double stage(double q, double) { return q; }
// up32(q): see the head of the file
__device__ __forceinline__ float stage(double q, float) {
  float f = (float)q;
  if ((double)f < q) {
    const uint32_t b = __float_as_uint(f);
    f = __uint_as_float(f == 0.0f ? 1u : (b >> 31 ? b - 1 : b + 1));
  }
  return f;
}

__global__ void __launch_bounds__(kBlock) k_clear64(unsigned long long* p, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) p[i] = 0;
}

// --- ranks, register form -------------------------------------------------------------

// Rows [lo, hi) of block x, the group of block y.  queries: F x Q float64,
// ascending per feature.  out: F x Q 64-bit sums, cleared before.
template <class T, int QP>
__global__ void __launch_bounds__(kBlock) k_ranks_reg(const T* __restrict__ x, uint64_t rows, uint64_t F, uint64_t len,
                                                      const double* __restrict__ queries, int Q, Abnormal ab, int fg,
                                                      unsigned long long* __restrict__ out) {
  __shared__ uint32_t acc[64 * QP];
  for (int i = threadIdx.x; i < 64 * QP; i += kBlock) acc[i] = 0;
  const Lane l = lane_of(F, fg);
  const Sieve<T> sieve(ab);
  T q[QP];
  uint32_t cnt[QP];
#pragma unroll
  for (int j = 0; j < QP; j++) {
    q[j] = j < Q ? stage(queries[(l.f0 + l.col) * Q + j], T()) : (T)__builtin_nan("");
    cnt[j] = 0;
  }
  const uint64_t lo = (uint64_t)blockIdx.x * len;
  const uint64_t hi = lo + len < rows ? lo + len : rows;
  const T* px = x + l.f0 + l.col;
  const uint64_t stride = (uint64_t)kWaves * l.rps * kUnroll;
  for (uint64_t rb = lo + (uint64_t)(threadIdx.x >> 6) * l.rps; rb < hi; rb += stride) {
    T v[kUnroll];
    load_steps(px, F, rb, hi, l, v);
#pragma unroll
    for (int u = 0; u < kUnroll; u++) {
      const T e = sieve(v[u]);  // NaN, abnormal, idle: below no query point
#pragma unroll
      for (int j = 0; j < QP; j++) cnt[j] += e < q[j] ? 1u : 0u;
    }
  }
#pragma unroll
  for (int j = 0; j < QP; j++) cnt[j] = column_sum(cnt[j], l);
  __syncthreads();
  if (l.row == 0) {
#pragma unroll
    for (int j = 0; j < QP; j++)
      if (cnt[j]) atomicAdd(&acc[l.col * QP + j], cnt[j]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < l.w * QP; i += kBlock) {
    const int c = i / QP, j = i - c * QP;
    if (j < Q && acc[i]) atomicAdd(&out[(l.f0 + c) * Q + j], (unsigned long long)acc[i]);
  }
}

// --- ranks, LDS form --------------------------------------------------------------------

// the number of the p - 1 table entries <= v (sa_hist.hip's code_of for T)
template <class T>
__device__ __forceinline__ uint32_t count_le(const T* tab, int p, T v) {
  uint32_t pos = 0;
  for (int step = p >> 1; step > 0; step >>= 1) pos += tab[pos + step - 1] <= v ? step : 0;
  return pos;
}

// LDS: the group's tables, fg x P of T, then the counters, fg x P of 32 bits,
// [column][c].  P: the power of two above Q.
template <class T>
__global__ void __launch_bounds__(kBlock) k_ranks_lds(const T* __restrict__ x, uint64_t rows, uint64_t F, uint64_t len,
                                                      const double* __restrict__ queries, int Q, int P, Abnormal ab,
                                                      int fg, unsigned long long* __restrict__ out) {
  extern __shared__ unsigned long long lds[];
  T* tab = reinterpret_cast<T*>(lds);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(tab + fg * P);
  const Lane l = lane_of(F, fg);
  const Sieve<T> sieve(ab);
  for (int i = threadIdx.x; i < l.w * P; i += kBlock) {
    const int c = i / P, e = i - c * P;
    tab[i] = e < Q ? stage(queries[(l.f0 + c) * Q + e], T()) : (T)__builtin_nan("");
    cnt[i] = 0;
  }
  __syncthreads();
  const uint64_t lo = (uint64_t)blockIdx.x * len;
  const uint64_t hi = lo + len < rows ? lo + len : rows;
  const T* px = x + l.f0 + l.col;
  const T* mine = tab + l.col * P;
  uint32_t* mycnt = cnt + l.col * P;
  const uint64_t stride = (uint64_t)kWaves * l.rps * kUnroll;
  for (uint64_t rb = lo + (uint64_t)(threadIdx.x >> 6) * l.rps; rb < hi; rb += stride) {
    T v[kUnroll];
    load_steps(px, F, rb, hi, l, v);
#pragma unroll
    for (int u = 0; u < kUnroll; u++) {
      const T e = sieve(v[u]);
      if (e == e) atomicAdd(&mycnt[count_le(mine, P, e)], 1u);  // c <= P - 1
    }
  }
  __syncthreads();
  // rank[j] = #{c <= j}: a wave a column, 64 codes a turn
  const int lane = threadIdx.x & 63;
  for (int c = threadIdx.x >> 6; c < l.w; c += kWaves) {
    uint32_t carry = 0;
    for (int base = 0; base < P; base += 64) {
      const int e = base + lane;
      uint32_t s = e < P ? cnt[c * P + e] : 0;
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)s, off, 64);
        if (lane >= off) s += t;
      }
      s += carry;
      carry = (uint32_t)__shfl((int)s, 63, 64);
      if (e < Q && s) atomicAdd(&out[(l.f0 + c) * Q + e], (unsigned long long)s);
    }
  }
}

// --- range ----------------------------------------------------------------------------------

// out: per feature four 64-bit words: min, max, count, missing.  While the
// pass runs min and max are ordered keys of the float64 values (an unsigned
// compare of keys is the compare of the values), combined with integer
// atomics; k_range_done turns them into float64.
__device__ __forceinline__ unsigned long long key_of(double d) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(d);
  return b >> 63 ? ~b : b | 1ull << 63;
}
__device__ __forceinline__ double value_of(unsigned long long k) {
  return __longlong_as_double((long long)(k >> 63 ? k ^ 1ull << 63 : ~k));
}

__global__ void __launch_bounds__(kBlock) k_range_init(unsigned long long* out, uint64_t F) {
  const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f < F) out[4 * f] = ~0ull, out[4 * f + 1] = 0, out[4 * f + 2] = 0, out[4 * f + 3] = 0;
}

__global__ void __launch_bounds__(kBlock) k_range_done(unsigned long long* out, uint64_t F) {
  const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= F) return;
  double mn = __builtin_inf(), mx = -__builtin_inf();
  if (out[4 * f + 2]) mn = value_of(out[4 * f]), mx = value_of(out[4 * f + 1]);
  mn = mn == 0.0 ? 0.0 : mn;  // a zero is +0.0
  mx = mx == 0.0 ? 0.0 : mx;
  out[4 * f] = (unsigned long long)__double_as_longlong(mn);
  out[4 * f + 1] = (unsigned long long)__double_as_longlong(mx);
}

template <class T>
__global__ void __launch_bounds__(kBlock) k_range(const T* __restrict__ x, uint64_t rows, uint64_t F, uint64_t len,
                                                  Abnormal ab, int fg, unsigned long long* __restrict__ out) {
  __shared__ T smn[kWaves][64], smx[kWaves][64];
  __shared__ uint32_t sn[kWaves][64], sm[kWaves][64];
  const Lane l = lane_of(F, fg);
  const Sieve<T> sieve(ab);
  const T inf = (T)__builtin_inf();
  T mn = inf, mx = -inf;
  uint32_t n = 0, miss = 0;
  const uint64_t lo = (uint64_t)blockIdx.x * len;
  const uint64_t hi = lo + len < rows ? lo + len : rows;
  const T* px = x + l.f0 + l.col;
  const uint64_t stride = (uint64_t)kWaves * l.rps * kUnroll;
  for (uint64_t rb = lo + (uint64_t)(threadIdx.x >> 6) * l.rps; rb < hi; rb += stride) {
    T v[kUnroll];
    const uint32_t ok = load_steps(px, F, rb, hi, l, v);
#pragma unroll
    for (int u = 0; u < kUnroll; u++) {
      const bool in = ok >> u & 1;
      miss += in && v[u] != v[u] ? 1u : 0u;
      const T e = sieve(v[u]);
      const bool good = in && e == e;
      n += good ? 1u : 0u;
      mn = good && e < mn ? e : mn;
      mx = good && e > mx ? e : mx;
    }
  }
  // the lanes of a column, then the block's waves, then one block's word a column
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s = 1; s < l.rps; s <<= 1) {
    const T a = __shfl_down(mn, s * l.w, 64), b = __shfl_down(mx, s * l.w, 64);
    const uint32_t c = (uint32_t)__shfl_down((int)n, s * l.w, 64), d = (uint32_t)__shfl_down((int)miss, s * l.w, 64);
    if (lane + s * l.w < 64) mn = a < mn ? a : mn, mx = b > mx ? b : mx, n += c, miss += d;
  }
  smn[wave][lane] = mn, smx[wave][lane] = mx, sn[wave][lane] = n, sm[wave][lane] = miss;
  __syncthreads();
  if (threadIdx.x < (unsigned)l.w) {
    const int c = threadIdx.x;  // row 0 of wave 0's layout: lane c is column c
    mn = inf, mx = -inf, n = 0, miss = 0;
    for (int wv = 0; wv < kWaves; wv++) {
      mn = smn[wv][c] < mn ? smn[wv][c] : mn, mx = smx[wv][c] > mx ? smx[wv][c] : mx;
      n += sn[wv][c], miss += sm[wv][c];
    }
    unsigned long long* o = out + 4 * (l.f0 + c);
    if (n) {
      atomicMin(&o[0], key_of((double)mn));
      atomicMax(&o[1], key_of((double)mx));
      atomicAdd(&o[2], (unsigned long long)n);
    }
    if (miss) atomicAdd(&o[3], (unsigned long long)miss);
  }
}

// --- checks -------------------------------------------------------------------------------------

static int check_shape(int x_type, uint64_t rows, uint64_t F, const char* what) {
  const int rc = check_float(x_type, what);
  if (rc != SA_OK) return rc;
  if (rows >> 40 || F >> 16) {  // a grid's y dimension takes the column groups
    sa_set_error("%s: rows must be below 2^40 and n_features below 2^16", what);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

static int check_q(int q, const char* what) {
  if (q < 1 || q > kMaxQ) {
    sa_set_error("%s: q must be in 1..%d", what, kMaxQ);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

static int take_abnormal(const double* abnormal, int n, const char* what, Abnormal* ab) {
  if (n < 0 || n > kMaxAbnormal || (n && !abnormal)) {
    sa_set_error("%s: n_abnormal must be in 0..%d, with abnormal given", what, kMaxAbnormal);
    return SA_ERR_ARG;
  }
  ab->n = n;
  for (int i = 0; i < kMaxAbnormal; i++) ab->v[i] = i < n ? abnormal[i] : __builtin_nan("");
  return SA_OK;
}

}  // namespace bin
}  // namespace sa

using namespace sa::bin;

extern "C" int sa_bin_geometry(int q, uint64_t n_features, int x_type, int* out5) {
  int rc = check_shape(x_type, 0, n_features, "sa_bin_geometry");
  if (rc == SA_OK) rc = check_q(q, "sa_bin_geometry");
  if (rc != SA_OK) return rc;
  if (n_features < 1 || !out5) {
    sa_set_error("sa_bin_geometry: at least one feature, and out5 is required");
    return SA_ERR_ARG;
  }
  const Geometry g = bin_geometry(q, n_features, (int)elem_size(x_type));
  out5[0] = g.form, out5[1] = g.qp, out5[2] = g.fg, out5[3] = g.lds, out5[4] = g.groups;
  return SA_OK;
}

extern "C" int sa_bin_range(const void* x, int x_type, uint64_t rows, uint64_t n_features, const double* abnormal,
                            int n_abnormal, void* out, void* stream) {
  int rc = check_shape(x_type, rows, n_features, "sa_bin_range");
  Abnormal ab;
  if (rc == SA_OK) rc = take_abnormal(abnormal, n_abnormal, "sa_bin_range", &ab);
  if (rc != SA_OK) return rc;
  if (n_features == 0) return SA_OK;
  if (!out || misaligned(out, 8) || (rows && (!x || misaligned(x, elem_size(x_type))))) {
    sa_set_error("sa_bin_range: bad arguments (x and out are required; element-aligned x, 8-byte aligned out)");
    return SA_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* o = (unsigned long long*)out;
  const unsigned fblocks = (unsigned)((n_features + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(k_range_init, dim3(fblocks), dim3(kBlock), 0, st, o, n_features);
  if (rows) {
    const Geometry g = bin_geometry(1, n_features, (int)elem_size(x_type));  // the register form's groups
    const Rows r = rows_grid(rows, g.fg, g.groups);
    dispatch_float(x_type, [&](auto t) {
      typedef decltype(t) T;
      hipLaunchKernelGGL(k_range<T>, dim3((unsigned)r.tiles, (unsigned)g.groups), dim3(kBlock), 0, st, (const T*)x, rows,
                         n_features, r.len, ab, g.fg, o);
    });
  }
  hipLaunchKernelGGL(k_range_done, dim3(fblocks), dim3(kBlock), 0, st, o, n_features);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

template <class T>
static void launch_reg(const Geometry& g, dim3 grid, hipStream_t st, const T* x, uint64_t rows, uint64_t F, uint64_t len,
                       const double* queries, int q, const Abnormal& ab, unsigned long long* out) {
  if (g.qp == 4)
    hipLaunchKernelGGL((k_ranks_reg<T, 4>), grid, dim3(kBlock), 0, st, x, rows, F, len, queries, q, ab, g.fg, out);
  else if (g.qp == 8)
    hipLaunchKernelGGL((k_ranks_reg<T, 8>), grid, dim3(kBlock), 0, st, x, rows, F, len, queries, q, ab, g.fg, out);
  else
    hipLaunchKernelGGL((k_ranks_reg<T, 16>), grid, dim3(kBlock), 0, st, x, rows, F, len, queries, q, ab, g.fg, out);
}

extern "C" int sa_bin_ranks(const void* x, int x_type, uint64_t rows, uint64_t n_features, const double* queries, int q,
                            const double* abnormal, int n_abnormal, int64_t* ranks_out, void* stream) {
  int rc = check_shape(x_type, rows, n_features, "sa_bin_ranks");
  if (rc == SA_OK) rc = check_q(q, "sa_bin_ranks");
  Abnormal ab;
  if (rc == SA_OK) rc = take_abnormal(abnormal, n_abnormal, "sa_bin_ranks", &ab);
  if (rc != SA_OK) return rc;
  if (n_features == 0) return SA_OK;
  if (!ranks_out || misaligned(ranks_out, 8) ||
      (rows && (!x || misaligned(x, elem_size(x_type)) || !queries || misaligned(queries, 8)))) {
    sa_set_error("sa_bin_ranks: bad arguments (x, queries and ranks_out are required; element-aligned x, 8-byte "
                 "aligned queries and ranks_out)");
    return SA_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* o = (unsigned long long*)ranks_out;
  const uint64_t cells = n_features * (uint64_t)q;
  hipLaunchKernelGGL(k_clear64, dim3((unsigned)((cells + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, o, cells);
  if (rows) {
    const Geometry g = bin_geometry(q, n_features, (int)elem_size(x_type));
    const Rows r = rows_grid(rows, g.fg, g.groups);
    const dim3 grid((unsigned)r.tiles, (unsigned)g.groups);
    dispatch_float(x_type, [&](auto t) {
      typedef decltype(t) T;
      if (g.form == 0)
        launch_reg<T>(g, grid, st, (const T*)x, rows, n_features, r.len, queries, q, ab, o);
      else
        hipLaunchKernelGGL(k_ranks_lds<T>, grid, dim3(kBlock), (size_t)g.lds, st, (const T*)x, rows, n_features, r.len,
                           queries, q, g.qp, ab, g.fg, o);
    });
  }
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}
