// sa_scr.hip — structure-wise update pruning (the reference's SCRSparse,
// sfl/utils/compressor/sparse_compressor.py:182-230, with the update and the
// residual of fed_scr.py:97-125 around it) as one stream-ordered sequence of
// launches over a tensor seen as [rows, cols, inner]:
//
//   u      = (a - b) + r                     materialised once (res_out, or
//                                            sparse_out when there is no res_out)
//   S0[i]  = float64 sum of |u[i,:,:]|;  row i dropped iff S0[i] / max(S0) <= thr
//   S1[j]  = float64 sum of |u[i,j,:]| over the kept rows;  column j likewise
//   sparse = u with the dropped rows and columns +0;  res = u - sparse
//
// max() propagates NaN (np.max), the ratio is a real float64 division, and
// every special case of the definition in include/sfl_sa.h follows from IEEE
// arithmetic.  The sums have one order per shape: a wave owns one segment of
// one row, its lanes add their own elements tile by tile, a butterfly joins
// the lanes, and one thread joins a row's segments in index order; a thread
// of the column pass owns four positions of the row and walks a slab of
// rows, and one thread per column joins slabs and inner positions.  Dropped
// rows are skipped, which for sums of magnitudes equals adding +0.  No float
// atomics, no allocation, no host synchronisation; maxima, flags and counts
// stay in device memory.
#include <hip/hip_runtime.h>

#include "sa_compress.h"

namespace sa {
namespace scr {

using namespace sa::elems;
using namespace sa::entry;
using sa::wave::kBlock;
using sa::wave::kWaves;

constexpr uint32_t kSeg = 8 * kTile;         // elements of a row per wave (form, apply)
constexpr uint32_t kSpan = kBlock * kEpl;    // positions of the row per block (column sums)
constexpr uint32_t kWide = 64;               // rows from this length on take the wave-per-segment kernels
constexpr uint32_t kColBlocks = 2048;        // blocks the column sums aim at: 8 per CU on 256 CUs

struct State {
  double m0, m1;               // max(S0), max(S1)
  uint32_t drop_rows, drop_cols;
  uint64_t pad[5];
};
static_assert(sizeof(State) == 64, "scratch layout");

// Where things lie in scratch; a function of the shape only.
struct Layout {
  uint64_t L;        // cols * inner: the row's length
  uint32_t segs;     // segments per row (1 on the narrow path)
  uint32_t tiles;    // blocks along the row in the column sums
  uint32_t slabs;    // slabs of rows in the column sums
  uint32_t slab_rows;
  uint64_t off_part, off_colpart, off_s1, off_rowflag, off_colflag, bytes;
};

static Layout layout(uint64_t R, uint64_t C, uint64_t K) {
  Layout y;
  y.L = C * K;
  y.segs = y.L >= kWide ? (uint32_t)((y.L + kSeg - 1) / kSeg) : 1;
  y.tiles = (uint32_t)((y.L + kSpan - 1) / kSpan);
  uint64_t want = (kColBlocks + y.tiles - 1) / y.tiles;
  if (want > R) want = R;
  y.slab_rows = (uint32_t)((R + want - 1) / want);
  y.slabs = (uint32_t)((R + y.slab_rows - 1) / y.slab_rows);
  auto up8 = [](uint64_t v) { return (v + 7) & ~(uint64_t)7; };
  y.off_part = sizeof(State);
  y.off_colpart = y.off_part + R * y.segs * sizeof(double);
  y.off_s1 = y.off_colpart + (uint64_t)y.slabs * y.L * sizeof(double);
  y.off_rowflag = y.off_s1 + C * sizeof(double);
  y.off_colflag = y.off_rowflag + up8(R);
  y.bytes = y.off_colflag + up8(C);
  return y;
}

template <class T>
__device__ __forceinline__ double mag(T x) {
  return fabs((double)x);
}

// np.max's maximum: a NaN operand wins
__device__ __forceinline__ double nanmax(double a, double b) {
  return a != a ? a : (b != b ? b : (a > b ? a : b));
}

// the wave's (row, segment): waves in (row, segment) order
struct Unit {
  uint64_t base;     // index of the row's first element
  uint32_t row, lo, hi;  // positions [lo, hi) of the row
  int lane;
  bool on;
};
__device__ __forceinline__ Unit wave_unit(uint32_t R, uint32_t L, uint32_t segs) {
  const uint64_t w = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  Unit u;
  u.on = w < (uint64_t)R * segs;
  u.row = (uint32_t)(w / segs);
  const uint32_t seg = (uint32_t)(w - (uint64_t)u.row * segs);
  u.base = (uint64_t)u.row * L;
  const uint64_t lo = (uint64_t)seg * kSeg, hi = lo + kSeg;
  u.lo = (uint32_t)lo;
  u.hi = hi < L ? (uint32_t)hi : L;
  u.lane = threadIdx.x & 63;
  return u;
}

template <class T>
__device__ __forceinline__ T form_one(const T* a, const T* b, const T* r, uint64_t i) {
  T u = a[i];
  if (b) u = u - b[i];
  if (r) u = u + r[i];
  return u;
}

// --- kernels --------------------------------------------------------------

// u = (a - b) + r -> u_out (may alias r); part[row * segs + seg] = the
// segment's float64 sum of |u|
template <class T>
__global__ void __launch_bounds__(kBlock) k_form(const T* __restrict__ a, const T* __restrict__ b, const T* r,
                                                 T* u_out, uint32_t R, uint32_t L, uint32_t segs, int vec,
                                                 double* __restrict__ part) {
  const Unit w = wave_unit(R, L, segs);
  if (!w.on) return;
  double acc = 0.0;
  for (uint64_t t = w.lo; t < w.hi; t += kTile) {
    const uint64_t p0 = t + (uint32_t)w.lane * kEpl;
    const int cnt = lane_count(p0, w.hi);
    const uint64_t e0 = w.base + p0;
    Elems<T> u = load_elems(a, e0, cnt, vec);
    if (b) {
      const Elems<T> y = load_elems(b, e0, cnt, vec);
#pragma unroll
      for (int j = 0; j < kEpl; j++) u.v[j] = u.v[j] - y.v[j];
    }
    if (r) {
      const Elems<T> y = load_elems(r, e0, cnt, vec);
#pragma unroll
      for (int j = 0; j < kEpl; j++) u.v[j] = u.v[j] + y.v[j];
    }
    store_elems(u_out, e0, cnt, vec, u);
#pragma unroll
    for (int j = 0; j < kEpl; j++)
      if (j < cnt) acc += mag(u.v[j]);
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (w.lane == 0) part[(uint64_t)w.row * segs + (w.lo / kSeg)] = acc;
}

// rows shorter than a wave: one thread per row
template <class T>
__global__ void __launch_bounds__(kBlock) k_form_narrow(const T* __restrict__ a, const T* __restrict__ b,
                                                        const T* r, T* u_out, uint32_t R, uint32_t L,
                                                        double* __restrict__ part) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= R) return;
  double acc = 0.0;
  for (uint32_t p = 0; p < L; p++) {
    const T u = form_one(a, b, r, i * L + p);
    u_out[i * L + p] = u;
    acc += mag(u);
  }
  part[i] = acc;
}

// One block.  sums[i * nseg + 0 .. nseg) are joined in index order into
// sums[i * nseg]; M = their NaN-propagating maximum; flags[i] = the ratio
// sums[i] / M is <= thr (a real division: 0/0 and inf/inf are NaN and keep).
__global__ void __launch_bounds__(kBlock) k_flags(double* sums, uint32_t nseg, uint32_t count, double thr,
                                                  uint8_t* __restrict__ flags, double* m_out, uint32_t* dropped_out,
                                                  uint32_t* stats_slot) {
  __shared__ double wmax[kWaves];
  __shared__ uint32_t wcnt[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double m = -1.0;  // below every sum of magnitudes
  for (uint64_t i = threadIdx.x; i < count; i += kBlock) {
    double s = sums[i * nseg];
    for (uint32_t g = 1; g < nseg; g++) s += sums[i * nseg + g];
    sums[i * nseg] = s;
    m = nanmax(m, s);
  }
  for (int off = 32; off > 0; off >>= 1) m = nanmax(m, __shfl_xor(m, off, 64));
  if (lane == 0) wmax[wave] = m;
  __syncthreads();
  m = nanmax(nanmax(wmax[0], wmax[1]), nanmax(wmax[2], wmax[3]));
  uint32_t c = 0;
  for (uint64_t i = threadIdx.x; i < count; i += kBlock) {
    const bool drop = sums[i * nseg] / m <= thr;
    flags[i] = drop ? 1 : 0;
    c += drop ? 1u : 0u;
  }
  for (int off = 32; off > 0; off >>= 1) c += (uint32_t)__shfl_xor((int)c, off, 64);
  if (lane == 0) wcnt[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    c = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
    *m_out = m;
    *dropped_out = c;
    if (stats_slot) *stats_slot = c;
  }
}

// colpart[slab * L + p] = float64 sum of |u[i, p]| over the slab's kept rows
// i, in row order.  A thread owns the positions [p0, p0 + 4) of every row.
template <class T>
__global__ void __launch_bounds__(kBlock) k_colsum(const T* __restrict__ u, uint32_t R, uint32_t L, uint32_t tiles,
                                                   uint32_t slab_rows, int vec,
                                                   const uint8_t* __restrict__ rowflag,
                                                   double* __restrict__ colpart) {
  const uint32_t slab = blockIdx.x / tiles, tile = blockIdx.x - slab * tiles;
  const uint64_t p0 = (uint64_t)tile * kSpan + threadIdx.x * kEpl;
  const int cnt = lane_count(p0, L);
  const uint32_t r0 = slab * slab_rows;
  const uint32_t r1 = R - r0 < slab_rows ? R : r0 + slab_rows;
  double acc[kEpl] = {0.0, 0.0, 0.0, 0.0};
  for (uint32_t i = r0; i < r1; i++) {
    if (rowflag[i]) continue;  // the same for every thread of the block
    const Elems<T> x = load_elems(u, (uint64_t)i * L + p0, cnt, vec);
#pragma unroll
    for (int j = 0; j < kEpl; j++) acc[j] += mag(x.v[j]);
  }
#pragma unroll
  for (int j = 0; j < kEpl; j++)
    if (j < cnt) colpart[(uint64_t)slab * L + p0 + j] = acc[j];
}

// s1[j] = the column's slabs and inner positions, joined slab by slab
__global__ void __launch_bounds__(kBlock) k_coljoin(const double* __restrict__ colpart, uint32_t C, uint32_t K,
                                                    uint32_t slabs, double* __restrict__ s1) {
  const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= C) return;
  const uint64_t L = (uint64_t)C * K;
  double s = 0.0;
  for (uint32_t g = 0; g < slabs; g++)
    for (uint32_t k = 0; k < K; k++) s += colpart[g * L + j * K + k];
  s1[j] = s;
}

// the column flags of the lane's positions [p0, p0 + 4)
struct Drop4 {
  bool d[kEpl];
  bool any;
};
__device__ __forceinline__ Drop4 col_drops(const uint8_t* __restrict__ colflag, uint32_t p0, int cnt, uint32_t K) {
  Drop4 f;
  if (K == 1 && cnt == kEpl) {  // p0 is a multiple of 4 and the flags are 8-byte aligned
    const uint32_t wd = *reinterpret_cast<const uint32_t*>(colflag + p0);
#pragma unroll
    for (int j = 0; j < kEpl; j++) f.d[j] = (wd >> (8 * j)) & 0xffu;
    f.any = wd != 0;
  } else {
    uint32_t c = p0 / K, rem = p0 - c * K;
    f.any = false;
#pragma unroll
    for (int j = 0; j < kEpl; j++) {
      f.d[j] = j < cnt && colflag[c];
      f.any |= f.d[j];
      if (++rem == K) rem = 0, c++;
    }
  }
  return f;
}

// RES: u lies in res; sparse = u with the dropped structures +0 and
// res = u - sparse.  A dropped element is never NaN (a NaN keeps everything),
// so u - 0 is u: a dropped row's residual is left as formed.
// !RES: u lies in sparse; the dropped structures are overwritten with +0.
template <class T, bool RES>
__global__ void __launch_bounds__(kBlock) k_apply(T* __restrict__ sparse, T* __restrict__ res, uint32_t R,
                                                  uint32_t L, uint32_t K, uint32_t segs, int vec,
                                                  const uint8_t* __restrict__ rowflag,
                                                  const uint8_t* __restrict__ colflag) {
  const Unit w = wave_unit(R, L, segs);
  if (!w.on) return;
  const bool rowdrop = rowflag[w.row];
  Elems<T> zero;
#pragma unroll
  for (int j = 0; j < kEpl; j++) zero.v[j] = T(0);
  for (uint64_t t = w.lo; t < w.hi; t += kTile) {
    const uint64_t p0 = t + (uint32_t)w.lane * kEpl;
    const int cnt = lane_count(p0, w.hi);
    const uint64_t e0 = w.base + p0;
    if (rowdrop) {
      store_elems(sparse, e0, cnt, vec, zero);
      continue;
    }
    if (cnt == 0) continue;
    const Drop4 f = col_drops(colflag, (uint32_t)p0, cnt, K);  // cnt > 0: p0 < L
    if (RES) {
      Elems<T> x = load_elems(res, e0, cnt, vec), sp;
#pragma unroll
      for (int j = 0; j < kEpl; j++) {
        sp.v[j] = f.d[j] ? T(0) : x.v[j];
        x.v[j] = x.v[j] - sp.v[j];
      }
      store_elems(sparse, e0, cnt, vec, sp);
      store_elems(res, e0, cnt, vec, x);
    } else if (f.any) {
#pragma unroll
      for (int j = 0; j < kEpl; j++)
        if (j < cnt && f.d[j]) sparse[e0 + j] = T(0);
    }
  }
}

template <class T, bool RES>
__global__ void __launch_bounds__(kBlock) k_apply_narrow(T* __restrict__ sparse, T* __restrict__ res, uint32_t R,
                                                         uint32_t L, uint32_t K,
                                                         const uint8_t* __restrict__ rowflag,
                                                         const uint8_t* __restrict__ colflag) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= R) return;
  const bool rowdrop = rowflag[i];
  uint32_t c = 0, rem = 0;
  for (uint32_t p = 0; p < L; p++) {
    const bool drop = rowdrop || colflag[c];
    if (++rem == K) rem = 0, c++;
    const uint64_t e = i * L + p;
    if (RES) {
      const T x = res[e];
      const T sp = drop ? T(0) : x;
      sparse[e] = sp;
      res[e] = x - sp;
    } else if (drop) {
      sparse[e] = T(0);
    }
  }
}

template <class T>
static int launch(const T* a, const T* b, const T* r, uint32_t R, uint32_t C, uint32_t K, double thr, T* sparse,
                  T* res, uint32_t* stats, char* scratch, hipStream_t s) {
  const Layout y = layout(R, C, K);
  const uint32_t L = (uint32_t)y.L;
  State* st = reinterpret_cast<State*>(scratch);
  double* part = reinterpret_cast<double*>(scratch + y.off_part);
  double* colpart = reinterpret_cast<double*>(scratch + y.off_colpart);
  double* s1 = reinterpret_cast<double*>(scratch + y.off_s1);
  uint8_t* rowflag = reinterpret_cast<uint8_t*>(scratch + y.off_rowflag);
  uint8_t* colflag = reinterpret_cast<uint8_t*>(scratch + y.off_colflag);
  T* u = res ? res : sparse;

  // 16-byte accesses: every vector aligned and every row starting on 16 bytes
  const uintptr_t all = (uintptr_t)a | (uintptr_t)b | (uintptr_t)r | (uintptr_t)sparse | (uintptr_t)res;
  const int vec = (all & 15) == 0 && (y.L * sizeof(T)) % 16 == 0;
  const bool wide = L >= kWide;
  const uint64_t units = (uint64_t)R * y.segs;
  const dim3 grid_rows((unsigned)(wide ? (units + kWaves - 1) / kWaves : ((uint64_t)R + kBlock - 1) / kBlock));

  if (wide)
    hipLaunchKernelGGL(k_form<T>, grid_rows, dim3(kBlock), 0, s, a, b, r, u, R, L, y.segs, vec, part);
  else
    hipLaunchKernelGGL(k_form_narrow<T>, grid_rows, dim3(kBlock), 0, s, a, b, r, u, R, L, part);
  SA_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_flags, dim3(1), dim3(kBlock), 0, s, part, y.segs, R, thr, rowflag, &st->m0, &st->drop_rows,
                     stats);
  SA_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_colsum<T>, dim3(y.tiles * y.slabs), dim3(kBlock), 0, s, (const T*)u, R, L, y.tiles,
                     y.slab_rows, vec, (const uint8_t*)rowflag, colpart);
  SA_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_coljoin, dim3((C + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const double*)colpart, C, K,
                     y.slabs, s1);
  SA_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_flags, dim3(1), dim3(kBlock), 0, s, s1, 1u, C, thr, colflag, &st->m1, &st->drop_cols,
                     stats ? stats + 1 : (uint32_t*)nullptr);
  SA_HIP_CHECK(hipGetLastError());
  if (wide) {
    if (res)
      hipLaunchKernelGGL((k_apply<T, true>), grid_rows, dim3(kBlock), 0, s, sparse, res, R, L, K, y.segs, vec,
                         (const uint8_t*)rowflag, (const uint8_t*)colflag);
    else
      hipLaunchKernelGGL((k_apply<T, false>), grid_rows, dim3(kBlock), 0, s, sparse, res, R, L, K, y.segs, vec,
                         (const uint8_t*)rowflag, (const uint8_t*)colflag);
  } else {
    if (res)
      hipLaunchKernelGGL((k_apply_narrow<T, true>), grid_rows, dim3(kBlock), 0, s, sparse, res, R, L, K,
                         (const uint8_t*)rowflag, (const uint8_t*)colflag);
    else
      hipLaunchKernelGGL((k_apply_narrow<T, false>), grid_rows, dim3(kBlock), 0, s, sparse, res, R, L, K,
                         (const uint8_t*)rowflag, (const uint8_t*)colflag);
  }
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

// SA_OK with the shape's layout, or SA_ERR_ARG with the error set
static int check_shape(const char* who, uint64_t R, uint64_t C, uint64_t K, int x_type, Layout* y) {
  if (check_float(x_type, who, "x_type") != SA_OK) return SA_ERR_ARG;
  if (R == 0 || C == 0 || K == 0) {
    sa_set_error("%s: rows, cols and inner must be positive", who);
    return SA_ERR_ARG;
  }
  if ((R >> 32) || (C >> 32) || (K >> 32) || ((C * K) >> 32) || ((R * (C * K)) >> 32)) {
    sa_set_error("%s: rows * cols * inner must be below 2^32 (indices and counts are 32-bit)", who);
    return SA_ERR_ARG;
  }
  *y = layout(R, C, K);
  if (y->bytes > 0x7fffffffull) {
    sa_set_error("%s: the shape needs 2 GiB of scratch or more", who);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

}  // namespace scr
}  // namespace sa

using namespace sa::scr;

extern "C" int sa_scr_scratch_bytes(uint64_t rows, uint64_t cols, uint64_t inner, int x_type) {
  Layout y;
  const int rc = check_shape("sa_scr_scratch_bytes", rows, cols, inner, x_type, &y);
  return rc != SA_OK ? rc : (int)y.bytes;
}

extern "C" int sa_scr(const void* a, const void* b, const void* r, int x_type, uint64_t rows, uint64_t cols,
                      uint64_t inner, double threshold, void* sparse_out, void* res_out, void* stats_out,
                      void* scratch, void* stream) {
  Layout y;
  const int rc = check_shape("sa_scr", rows, cols, inner, x_type, &y);
  if (rc != SA_OK) return rc;
  const uintptr_t esz = elem_size(x_type);
  const uintptr_t all = (uintptr_t)a | (uintptr_t)b | (uintptr_t)r | (uintptr_t)sparse_out | (uintptr_t)res_out;
  if (!a || !sparse_out || !scratch || (all & (esz - 1)) || ((uintptr_t)stats_out & 3) ||
      ((uintptr_t)scratch & 7)) {
    sa_set_error("sa_scr: bad arguments (a, sparse_out and scratch are required; element-aligned vectors, "
                 "4-byte aligned stats_out, 8-byte aligned scratch)");
    return SA_ERR_ARG;
  }
  if (sparse_out == a || sparse_out == b || sparse_out == r ||
      (res_out && (res_out == a || res_out == b || res_out == sparse_out))) {
    sa_set_error("sa_scr: only res_out may alias r");
    return SA_ERR_ARG;
  }
  return dispatch_float(x_type, [&](auto t) {
    typedef decltype(t) T;
    return launch((const T*)a, (const T*)b, (const T*)r, (uint32_t)rows, (uint32_t)cols, (uint32_t)inner, threshold,
                  (T*)sparse_out, (T*)res_out, (uint32_t*)stats_out, (char*)scratch, (hipStream_t)stream);
  });
}
