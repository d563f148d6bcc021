// sa_kmeans.hip — QuantizedKmeans on the device (the reference's class,
// sfl/utils/compressor/quantized_compressor.py:231-279, with the fit pinned:
// sfl_amd/utils/quantized.py has the definition).  A 1-D k-means run in
// integers on the 32-bit image u of the tensor:
//
//   hist    = the 4096-bin histogram of u >> 20, for the host's start
//   step    = one Lloyd step on the state block: an accumulate pass over the
//             tensor (cnt and sum per cluster), then one block that forms the
//             new centres, compares and clears the tables
//   labels  = the codes under the final centres, one streaming pass
//   lut     = codes -> values through q, one streaming pass
//
// Counts and sums are integers, added with integer atomics in LDS and in
// global memory: their result does not depend on the order, so the same input
// gives the same bits on every run and the bits of the numpy form.  No float
// atomics anywhere.  The image is computed anew in every pass (4 or 8 bytes
// read per element and step, nothing written).
//
// The accumulate and histogram passes run on sa_compress.h's contiguous wave
// layout; the two code passes on sa_runs.h's lane runs, as sa_quant_affine and
// sa_dequant_affine.
#include <hip/hip_runtime.h>

#include "sa_runs.h"

namespace sa {
namespace kmeans {

using namespace sa::elems;
using namespace sa::entry;
using namespace sa::runs;
using namespace sa::wave;

constexpr int kMaxK = SA_KMEANS_MAX_K;
constexpr int kBins = SA_KMEANS_BINS;
constexpr int kBinShift = 20;  // 2^32 / kBins
constexpr int kTable = 1024;   // LDS entries of a block's cnt / sum table: clusters x copies
// tiles a wave loads before it works on them, in the histogram and accumulate
// passes (a tile beyond the wave's range has no element and loads nothing)
constexpr int kInFlight = 4;

// the state block of a fit (include/sfl_sa.h states the layout: the caller writes it)
struct State {
  uint64_t sum[kMaxK];
  uint32_t cnt[kMaxK];
  uint32_t c[kMaxK];
  uint32_t done, n_iter;
};
static_assert(sizeof(State) == SA_KMEANS_STATE_BYTES, "state layout");
static_assert(offsetof(State, c) == SA_KMEANS_STATE_C && offsetof(State, done) == SA_KMEANS_STATE_DONE,
              "state layout");

// u = min(U, uint64(rint((float64(x) - mn) * s))), U = 2^32 - 1.  The
// subtraction and the multiplication round separately: contracted into an FMA
// the product would not be rounded and u could differ from numpy's by one.
// (A NaN or an x below mn, which the callers refuse, gives 0 or U: a value
// inside the image either way.)
template <class T>
__device__ __forceinline__ uint32_t image(T x, double mn, double s) {
#pragma clang fp contract(off)
  const double d = (double)x - mn;
  const double r = rint(d * s);
  return (uint32_t)fmin(fmax(r, 0.0), 4294967295.0);
}

// the smallest power of two >= k (k in 2..256)
__host__ __device__ __forceinline__ int pow2_of(int k) {
  int p = 2;
  while (p < k) p <<= 1;
  return p;
}

// The boundaries b_j = (c_j + c_{j+1}) >> 1, j < k - 1, into bnd[0 .. p - 2],
// the rest 2^32 - 1, which no u exceeds; p = pow2_of(k).  Ends with a barrier.
__device__ __forceinline__ void load_boundaries(const uint32_t* __restrict__ c, int k, int p, uint32_t* bnd) {
  for (int j = threadIdx.x; j < p - 1; j += kBlock)
    bnd[j] = j < k - 1 ? (uint32_t)(((uint64_t)c[j] + c[j + 1]) >> 1) : 0xffffffffu;
  __syncthreads();
}

// the number of j with b_j < u: a branch-free binary search over the p - 1
// sorted entries, log2(p) <= 8 probes; an element on a boundary stays below it
__device__ __forceinline__ uint32_t label_of(const uint32_t* bnd, int p, uint32_t u) {
  uint32_t pos = 0;
  for (int step = p >> 1; step > 0; step >>= 1) pos += bnd[pos + step - 1] < u ? step : 0;
  return pos;
}

// --- the start's histogram ---------------------------------------------------

template <class T>
__global__ void __launch_bounds__(kBlock) k_hist(const T* __restrict__ x, uint64_t n, uint64_t len, int vec, double mn,
                                                 double s, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[kBins];
  for (int i = threadIdx.x; i < kBins; i += kBlock) h[i] = 0;
  __syncthreads();
  const Range w = wave_range(n, len);
  for (uint64_t t = w.lo; t < w.hi; t += kInFlight * kTile) {
    Elems<T> v[kInFlight];
    int cnt[kInFlight];
#pragma unroll
    for (int i = 0; i < kInFlight; i++) {
      const uint64_t e0 = t + (uint64_t)i * kTile + (uint64_t)w.lane * kEpl;
      cnt[i] = lane_count(e0, w.hi);
      v[i] = load_elems(x, e0, cnt[i], vec);
    }
#pragma unroll
    for (int i = 0; i < kInFlight; i++) {
#pragma unroll
      for (int j = 0; j < kEpl; j++)
        if (j < cnt[i]) atomicAdd(&h[image(v[i].v[j], mn, s) >> kBinShift], 1u);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kBins; b += kBlock)
    if (h[b]) atomicAdd(&hist[b], h[b]);
}

// --- one Lloyd step ------------------------------------------------------------

// cnt_j and sum_j of this block's share into the state's tables.  The block's
// table has `copies` copies of every cluster (kTable / p, at most 64); lane l
// adds into copy l % copies at [label * copies + copy], so the lanes of one
// wave-instruction meet in one address `copies` times less often, and with 64
// copies every lane of a 32-bit add has a bank of its own.
template <class T>
__global__ void __launch_bounds__(kBlock) k_accumulate(const T* __restrict__ x, uint64_t n, uint64_t len, int vec,
                                                       double mn, double s, int k, State* __restrict__ st) {
  __shared__ unsigned long long lsum[kTable];
  __shared__ uint32_t lcnt[kTable];
  __shared__ uint32_t bnd[kMaxK];
  if (st->done) return;  // written by k_update only: the whole grid sees one value
  const int p = pow2_of(k);
  const int copies = kTable / p < 64 ? kTable / p : 64;
  for (int i = threadIdx.x; i < kTable; i += kBlock) lsum[i] = 0, lcnt[i] = 0;
  load_boundaries(st->c, k, p, bnd);
  const Range w = wave_range(n, len);
  const uint32_t copy = (uint32_t)w.lane & (uint32_t)(copies - 1);
  for (uint64_t t = w.lo; t < w.hi; t += kInFlight * kTile) {
    Elems<T> v[kInFlight];
    int cnt[kInFlight];
#pragma unroll
    for (int i = 0; i < kInFlight; i++) {
      const uint64_t e0 = t + (uint64_t)i * kTile + (uint64_t)w.lane * kEpl;
      cnt[i] = lane_count(e0, w.hi);
      v[i] = load_elems(x, e0, cnt[i], vec);
    }
#pragma unroll
    for (int i = 0; i < kInFlight; i++) {
#pragma unroll
      for (int j = 0; j < kEpl; j++) {
        if (j < cnt[i]) {
          const uint32_t u = image(v[i].v[j], mn, s);
          const uint32_t at = label_of(bnd, p, u) * copies + copy;  // label < k <= p: inside the table
          atomicAdd(&lcnt[at], 1u);
          atomicAdd(&lsum[at], (unsigned long long)u);
        }
      }
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < k; j += kBlock) {
    uint32_t c = 0;
    unsigned long long a = 0;
    for (int i = 0; i < copies; i++) c += lcnt[j * copies + i], a += lsum[j * copies + i];
    if (c) {
      atomicAdd(&st->cnt[j], c);
      atomicAdd(reinterpret_cast<unsigned long long*>(&st->sum[j]), a);
    }
  }
}

// One block: c'_j = round-half-up(sum_j / cnt_j), an empty cluster keeps c_j;
// done if no centre moved; n_iter += 1; the tables are left zeroed for the
// next step.
__global__ void __launch_bounds__(kBlock) k_update(int k, State* st) {
  const uint32_t done = st->done;
  __syncthreads();  // every thread has read `done` before thread 0 may write it
  if (done) return;
  int moved = 0;
  for (int j = threadIdx.x; j < k; j += kBlock) {
    const uint32_t c = st->c[j], cnt = st->cnt[j];
    const uint64_t sum = st->sum[j];
    uint32_t nc = c;
    if (cnt) {
      const uint64_t q = sum / cnt, r = sum % cnt;
      nc = (uint32_t)(q + (2 * r >= cnt ? 1 : 0));  // q == 2^32 - 1 only with r == 0
    }
    moved |= nc != c;
    st->c[j] = nc, st->cnt[j] = 0, st->sum[j] = 0;
  }
  moved = __syncthreads_or(moved);
  if (threadIdx.x == 0) {
    st->n_iter += 1;
    if (!moved) st->done = 1;
  }
}

// --- the codes --------------------------------------------------------------------

// code = label - offset under the centres st->c; sa_quant.hip's k_quant with
// the boundaries in LDS: elements [0, head) and [head + nruns * 16, n) are the
// scalar head and tail, taken by the first threads of block 0
template <class T, int QB>
__global__ void __launch_bounds__(kBlock) k_labels(const T* __restrict__ x, uint64_t n, uint32_t head, uint64_t nruns,
                                                   int vec, double mn, double s, int k, const State* __restrict__ st,
                                                   int offset, void* __restrict__ q) {
  __shared__ uint32_t bnd[kMaxK];
  const int p = pow2_of(k);
  load_boundaries(st->c, k, p, bnd);
  const uint64_t nthreads = (uint64_t)gridDim.x * kBlock;
  const T* xb = x + head;
  char* qb = reinterpret_cast<char*>(q) + (uint64_t)head * QB;
  for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < nruns; r += nthreads) {
    T v[kEncRun];
    load_run<T, kEncRun>(xb + r * kEncRun, v, vec);
    int32_t c[kEncRun];
#pragma unroll
    for (int j = 0; j < kEncRun; j++) c[j] = (int32_t)label_of(bnd, p, image(v[j], mn, s)) - offset;
    Codes<QB, kEncRun> out;
    out.pack(c);
    out.store(qb + r * kEncRun * QB);
  }
  if (blockIdx.x == 0) {
    const uint64_t t = threadIdx.x, tail0 = head + nruns * kEncRun;
    if (t < head) store_code<QB>(q, t, (int32_t)label_of(bnd, p, image(x[t], mn, s)) - offset);
    if (tail0 + t < n) store_code<QB>(q, tail0 + t, (int32_t)label_of(bnd, p, image(x[tail0 + t], mn, s)) - offset);
  }
}

// out[i] = lut[code[i] + offset].  A code whose label falls outside [0, k) is
// another party's data: it is never used as an index, the element becomes 0
// and the flag record gets SA_KMEANS_BAD_CODE and the least such position.
template <class T>
__device__ __forceinline__ T lut_value(const T* lut, int k, int32_t code, int offset, uint64_t i, uint32_t* flag) {
  const uint32_t label = (uint32_t)(code + offset);  // a negative label wraps above k
  if (label < (uint32_t)k) return lut[label];
  atomicOr(&flag[0], SA_KMEANS_BAD_CODE);
  atomicMin(&flag[1], (uint32_t)i);
  return T(0);
}

// sa_quant.hip's k_dequant with the values in LDS
template <class T, int QB>
__global__ void __launch_bounds__(kBlock) k_lut(const void* __restrict__ q, uint64_t n, uint32_t head, uint64_t nruns,
                                                int vec, const T* __restrict__ lut_in, int k, int offset,
                                                T* __restrict__ out, uint32_t* flag) {
  constexpr int kRun = kDecRun<T>, kUnroll = 16 / kRun;
  __shared__ T lut[kMaxK];
  for (int j = threadIdx.x; j < k; j += kBlock) lut[j] = lut_in[j];
  __syncthreads();
  const uint64_t nthreads = (uint64_t)gridDim.x * kBlock;
  T* ob = out + head;
  const char* qb = reinterpret_cast<const char*>(q) + (uint64_t)head * QB;
  for (uint64_t r0 = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r0 < nruns; r0 += nthreads * kUnroll) {
    Codes<QB, kRun> in[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; u++) {
      const uint64_t r = r0 + u * nthreads;
      if (r < nruns) in[u].load(qb + r * kRun * QB);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; u++) {
      const uint64_t r = r0 + u * nthreads;
      if (r < nruns) {
        int32_t c[kRun];
        in[u].unpack(c);
        T v[kRun];
#pragma unroll
        for (int j = 0; j < kRun; j++) v[j] = lut_value(lut, k, c[j], offset, head + r * kRun + j, flag);
        store_run<T, kRun>(ob + r * kRun, v, vec);
      }
    }
  }
  if (blockIdx.x == 0) {
    const uint64_t t = threadIdx.x, tail0 = head + nruns * kRun;
    if (t < head) out[t] = lut_value(lut, k, load_code<QB>(q, t), offset, t, flag);
    if (tail0 + t < n) out[tail0 + t] = lut_value(lut, k, load_code<QB>(q, tail0 + t), offset, tail0 + t, flag);
  }
}

// --- checks ----------------------------------------------------------------------

static int check_k(int k, const char* what) {
  if (k < 2 || k > kMaxK) {
    sa_set_error("%s: k must be in 2..256", what);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

// the labels' offset 2^(bits-1): k labels fit above it in the storage type
static int check_offset(int offset, int k, int q_bytes, const char* what) {
  const int lim = q_bytes == 1 ? 128 : 32768;
  if (offset < 1 || offset > lim || k - offset > lim) {
    sa_set_error("%s: label - offset must fit the codes' storage type for every label below k", what);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

static int check_x_state(const void* x, uintptr_t esz, uint64_t n, const void* state, const char* what) {
  if ((n && !x) || misaligned(x, esz) || !state || misaligned(state, 8)) {
    sa_set_error("%s: bad arguments (x and the state are required; element-aligned x, 8-byte aligned state)", what);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

}  // namespace kmeans
}  // namespace sa

using namespace sa::kmeans;

extern "C" int sa_kmeans_scratch_bytes(uint64_t n, int x_type) {
  const int rc = check_float_n(x_type, n, 32, "sa_kmeans_scratch_bytes");
  return rc == SA_OK ? (int)(kBins * sizeof(uint32_t) + sizeof(State)) : rc;
}

extern "C" int sa_kmeans_hist(const void* x, int x_type, uint64_t n, double mn, double s, void* hist, void* stream) {
  const int rc = check_float_n(x_type, n, 32, "sa_kmeans_hist");
  if (rc != SA_OK) return rc;
  if ((n && !x) || misaligned(x, elem_size(x_type)) || !hist || misaligned(hist, 4)) {
    sa_set_error("sa_kmeans_hist: bad arguments (x and hist are required; element-aligned x, 4-byte aligned hist)");
    return SA_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  SA_HIP_CHECK(hipMemsetAsync(hist, 0, kBins * sizeof(uint32_t), st));
  if (n == 0) return SA_OK;
  const Grid g = wave_grid(n, (uintptr_t)x);
  dispatch_float(x_type, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL(k_hist<T>, dim3(g.grid), dim3(kBlock), 0, st, (const T*)x, n, g.len, g.vec, mn, s,
                       (uint32_t*)hist);
  });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_kmeans_step(const void* x, int x_type, uint64_t n, double mn, double s, int k, int steps,
                              void* state, void* stream) {
  int rc = check_float_n(x_type, n, 32, "sa_kmeans_step");
  if (rc == SA_OK) rc = check_k(k, "sa_kmeans_step");
  if (rc == SA_OK) rc = check_x_state(x, elem_size(x_type), n, state, "sa_kmeans_step");
  if (rc != SA_OK) return rc;
  if (steps < 0) {
    sa_set_error("sa_kmeans_step: steps must not be negative");
    return SA_ERR_ARG;
  }
  if (steps == 0) return SA_OK;
  hipStream_t st = (hipStream_t)stream;
  const Grid g = wave_grid(n, (uintptr_t)x);
  for (int i = 0; i < steps; i++) {
    dispatch_float(x_type, [&](auto t) {
      typedef decltype(t) T;
      hipLaunchKernelGGL(k_accumulate<T>, dim3(g.grid), dim3(kBlock), 0, st, (const T*)x, n, g.len, g.vec, mn, s, k,
                         (State*)state);
    });
    hipLaunchKernelGGL(k_update, dim3(1), dim3(kBlock), 0, st, k, (State*)state);
  }
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_kmeans_labels(const void* x, int x_type, uint64_t n, double mn, double s, int k, const void* state,
                                int offset, void* q_out, int q_bytes, void* stream) {
  int rc = check_float_n(x_type, n, 32, "sa_kmeans_labels");
  if (rc == SA_OK) rc = check_k(k, "sa_kmeans_labels");
  if (rc == SA_OK) rc = check_vectors(x, elem_size(x_type), q_out, q_bytes, n, "sa_kmeans_labels");
  if (rc == SA_OK) rc = check_x_state(x, elem_size(x_type), n, state, "sa_kmeans_labels");
  if (rc == SA_OK) rc = check_offset(offset, k, q_bytes, "sa_kmeans_labels");
  if (rc != SA_OK) return rc;
  if (n == 0) return SA_OK;
  hipStream_t st = (hipStream_t)stream;
  dispatch_float(x_type, [&](auto t) {
    typedef decltype(t) T;
    if (q_bytes == 1) {
      const Plan p = plan_of(n, q_out, Codes<1, kEncRun>::kAlign, 1, x, sizeof(T), kEncRun, 1);
      hipLaunchKernelGGL((k_labels<T, 1>), dim3(p.grid), dim3(kBlock), 0, st, (const T*)x, n, p.head, p.nruns, p.vec, mn,
                         s, k, (const State*)state, offset, q_out);
    } else {
      const Plan p = plan_of(n, q_out, Codes<2, kEncRun>::kAlign, 2, x, sizeof(T), kEncRun, 1);
      hipLaunchKernelGGL((k_labels<T, 2>), dim3(p.grid), dim3(kBlock), 0, st, (const T*)x, n, p.head, p.nruns, p.vec, mn,
                         s, k, (const State*)state, offset, q_out);
    }
  });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_dequant_lut(const void* q, int q_bytes, uint64_t n, const void* lut, int k, int offset, int x_type,
                              void* out, void* flag, void* stream) {
  int rc = check_float_n(x_type, n, 32, "sa_dequant_lut");
  if (rc == SA_OK) rc = check_k(k, "sa_dequant_lut");
  const uintptr_t esz = elem_size(x_type);
  if (rc == SA_OK) rc = check_vectors(out, esz, q, q_bytes, n, "sa_dequant_lut");
  if (rc == SA_OK) rc = check_offset(offset, k, q_bytes, "sa_dequant_lut");
  if (rc != SA_OK) return rc;
  if (!lut || misaligned(lut, esz) || !flag || misaligned(flag, 4)) {
    sa_set_error("sa_dequant_lut: bad arguments (lut and flag are required; element-aligned lut, 4-byte aligned "
                 "flag)");
    return SA_ERR_ARG;
  }
  if (n == 0) return SA_OK;
  hipStream_t st = (hipStream_t)stream;
  dispatch_float(x_type, [&](auto t) {
    typedef decltype(t) T;
    constexpr int kRun = kDecRun<T>;
    if (q_bytes == 1) {
      const Plan p = plan_of(n, q, Codes<1, kRun>::kAlign, 1, out, sizeof(T), kRun, 16 / kRun);
      hipLaunchKernelGGL((k_lut<T, 1>), dim3(p.grid), dim3(kBlock), 0, st, q, n, p.head, p.nruns, p.vec, (const T*)lut,
                         k, offset, (T*)out, (uint32_t*)flag);
    } else {
      const Plan p = plan_of(n, q, Codes<2, kRun>::kAlign, 2, out, sizeof(T), kRun, 16 / kRun);
      hipLaunchKernelGGL((k_lut<T, 2>), dim3(p.grid), dim3(kBlock), 0, st, q, n, p.head, p.nruns, p.vec, (const T*)lut,
                         k, offset, (T*)out, (uint32_t*)flag);
    }
  });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}
