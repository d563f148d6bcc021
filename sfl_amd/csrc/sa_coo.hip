// sa_coo.hip — the COO transport of compressed updates on the device (the
// reference's sparse_encode / sparse_decode, sfl/utils/compressor/
// sparse_compressor.py:234-284, and the sum of its SparsePlainAggregator,
// sfl/security/aggregation/sparse_plain_aggregator.py:25-139):
//
//   encode  = count (pass 1 over x) + offsets (one block) + fill (pass 2)
//   decode  = zero the dense tensor, then a validated scatter
//   sum     = one validated axpy per party into a dense accumulator, then one
//             streaming division
//   gather  = a tensor's values at a validated index vector (the sparse_mask
//             path of sfl_amd/utils/sparse_compressor.py)
//
// A non-zero is decided on the bit pattern, (bits & ~sign) != 0.  The encode
// is a compaction in the wave layout that sa_stc uses too (sa_compress.h):
// every wave owns a CONTIGUOUS index range, so wave order is index order; a
// wave's first rank is the exclusive
// prefix of the per-wave counts, and inside a tile a lane's rank comes from
// three ballots over the lane counts (0..4).  No atomics and no sort: index_out
// is strictly ascending by construction.  A payload is another party's data:
// the scatter and the axpy never use an index outside [0, n) as an address and
// report what they met in a flag record.  Nothing is allocated, copied to the
// host or synchronised.
#include <hip/hip_runtime.h>

#include "sa_compress.h"

namespace sa {
namespace coo {

using namespace sa::elems;
using namespace sa::wave;  // the contiguous wave layout and the block scan
using namespace sa::entry;

// scratch: the per-wave counts, then (after k_offsets) each wave's first
// rank; one word more holds the total
constexpr size_t kScratchBytes = (kMaxWaves + 2) * sizeof(uint32_t);

template <class T>
struct Bits;
template <>
struct Bits<float> {
  static __device__ __forceinline__ bool nonzero(float x) { return (__float_as_uint(x) & 0x7fffffffu) != 0; }
};
template <>
struct Bits<double> {
  static __device__ __forceinline__ bool nonzero(double x) {
    return ((uint64_t)__double_as_longlong(x) & 0x7fffffffffffffffull) != 0;
  }
};

// --- encode -----------------------------------------------------------------

// pass 1: per wave, its non-zeros
template <class T>
__global__ void __launch_bounds__(kBlock) k_count(const T* __restrict__ x, uint64_t n, uint64_t len, int vec,
                                                  uint32_t* __restrict__ cnt) {
  const Range w = wave_range(n, len);
  uint32_t c = 0;
  for (uint64_t t = w.lo; t < w.hi; t += 2 * kTile) {
    const uint64_t e0 = t + (uint64_t)w.lane * kEpl, e1 = e0 + kTile;
    const int c0 = lane_count(e0, w.hi), c1 = lane_count(e1, w.hi);
    const Elems<T> x0 = load_elems(x, e0, c0, vec);
    const Elems<T> x1 = load_elems(x, e1, c1, vec);
#pragma unroll
    for (int j = 0; j < kEpl; j++) {
      c += (j < c0 && Bits<T>::nonzero(x0.v[j])) ? 1u : 0u;
      c += (j < c1 && Bits<T>::nonzero(x1.v[j])) ? 1u : 0u;
    }
  }
  for (int off = 32; off > 0; off >>= 1) c += (uint32_t)__shfl_xor((int)c, off, 64);
  if (w.lane == 0) cnt[blockIdx.x * kWaves + (threadIdx.x >> 6)] = c;
}

// One block: cnt -> exclusive prefix (each wave's first rank); the total
// into cnt[kMaxWaves] and nnz_out.
__global__ void __launch_bounds__(kBlock) k_offsets(uint32_t* cnt, int nwaves, uint32_t* __restrict__ nnz_out) {
  constexpr int PER = kMaxWaves / kBlock;
  uint32_t c[PER], s = 0;
#pragma unroll
  for (int j = 0; j < PER; j++) {
    const int i = threadIdx.x * PER + j;
    c[j] = i < nwaves ? cnt[i] : 0u;
    s += c[j];
  }
  uint32_t total;
  uint32_t run = block_scan_incl(s, &total) - s;
#pragma unroll
  for (int j = 0; j < PER; j++) {
    const int i = threadIdx.x * PER + j;
    if (i < nwaves) cnt[i] = run;
    run += c[j];
  }
  if (threadIdx.x == 0) {
    cnt[kMaxWaves] = total;
    *nnz_out = total;
  }
}

// pass 2: rank = the wave's first rank + the earlier tiles' count + the
// ballot prefix of the lane counts (lane-major, then j: index order)
template <class T>
__global__ void __launch_bounds__(kBlock) k_fill(const T* __restrict__ x, uint64_t n, uint64_t len, int vec,
                                                 const uint32_t* __restrict__ first, int32_t* __restrict__ index_out,
                                                 T* __restrict__ data_out, uint32_t cap, uint32_t* flag) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && first[kMaxWaves] != cap) atomicOr(&flag[0], (uint32_t)SA_COO_BAD_COUNT);
  const Range w = wave_range(n, len);
  uint32_t carry = first[blockIdx.x * kWaves + (threadIdx.x >> 6)];
  const uint64_t below = ((uint64_t)1 << w.lane) - 1;
  for (uint64_t t = w.lo; t < w.hi; t += kTile) {
    const uint64_t e0 = t + (uint64_t)w.lane * kEpl;
    const int cnt = lane_count(e0, w.hi);
    const Elems<T> v = load_elems(x, e0, cnt, vec);
    bool nz[kEpl];
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < kEpl; j++) {
      nz[j] = j < cnt && Bits<T>::nonzero(v.v[j]);
      c += nz[j] ? 1u : 0u;
    }
    if (__ballot(c != 0) == 0) continue;  // wave-uniform
    const uint64_t b0 = __ballot(c & 1u), b1 = __ballot(c & 2u), b2 = __ballot(c & 4u);
    uint32_t rank = carry + (uint32_t)__popcll(b0 & below) + 2u * (uint32_t)__popcll(b1 & below) +
                    4u * (uint32_t)__popcll(b2 & below);
    carry += (uint32_t)__popcll(b0) + 2u * (uint32_t)__popcll(b1) + 4u * (uint32_t)__popcll(b2);
#pragma unroll
    for (int j = 0; j < kEpl; j++) {
      if (nz[j]) {
        if (rank < cap) {
          index_out[rank] = (int32_t)(e0 + j);
          data_out[rank] = v.v[j];
        }
        rank++;
      }
    }
  }
}

// --- decode and the sparse sum -------------------------------------------------

// entry i: inside the tensor?  above its predecessor?  The verdicts go into
// the flag record; the return value says whether index[i] may be an address.
__device__ __forceinline__ bool check_entry(const int32_t* __restrict__ index, uint64_t i, uint32_t n,
                                            uint32_t* flag, uint32_t* at) {
  const int32_t k = index[i];
  const bool inside = (uint32_t)k < n;  // a negative index is >= 2^31 > n
  uint32_t bad = inside ? 0u : (uint32_t)SA_COO_BAD_RANGE;
  if (i > 0 && k <= index[i - 1]) bad |= (uint32_t)SA_COO_BAD_ORDER;
  if (bad) {
    atomicOr(&flag[0], bad);
    atomicMin(&flag[1], (uint32_t)i);
  }
  *at = (uint32_t)k;
  return inside;
}

template <class T>
__global__ void __launch_bounds__(kBlock) k_scatter(const int32_t* __restrict__ index, const T* __restrict__ data,
                                                    uint64_t nnz, uint32_t n, T* __restrict__ dense,
                                                    uint32_t* flag) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nnz; i += (uint64_t)gridDim.x * kBlock) {
    uint32_t at;
    if (check_entry(index, i, n, flag, &at)) dense[at] = data[i];
  }
}

// acc[index[i]] += A(data[i]) * w: multiply and add rounded separately
// (-ffp-contract=off).  A valid payload has unique indices, so no two threads
// meet in one element; an invalid one is flagged and its sum is unspecified.
template <class T, class A>
__global__ void __launch_bounds__(kBlock) k_axpy(const int32_t* __restrict__ index, const T* __restrict__ data,
                                                 uint64_t nnz, uint32_t n, A w, A* __restrict__ acc,
                                                 uint32_t* flag) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nnz; i += (uint64_t)gridDim.x * kBlock) {
    uint32_t at;
    if (check_entry(index, i, n, flag, &at)) {
      const A p = (A)data[i] * w;
      acc[at] = acc[at] + p;
    }
  }
}

// data_out[i] = x[index[i]]: the values of a tensor at a mask's positions
// (zeros included); the mask is validated like a payload
template <class T>
__global__ void __launch_bounds__(kBlock) k_gather(const int32_t* __restrict__ index, uint64_t nnz,
                                                   const T* __restrict__ x, uint32_t n, T* __restrict__ data_out,
                                                   uint32_t* flag) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nnz; i += (uint64_t)gridDim.x * kBlock) {
    uint32_t at;
    if (check_entry(index, i, n, flag, &at)) data_out[i] = x[at];
  }
}

template <class A>
__global__ void __launch_bounds__(kBlock) k_divide(A* acc, uint64_t n, uint64_t len, int vec, A d) {
  const Range w = wave_range(n, len);
  for (uint64_t t = w.lo; t < w.hi; t += kTile) {
    const uint64_t e0 = t + (uint64_t)w.lane * kEpl;
    const int cnt = lane_count(e0, w.hi);
    Elems<A> v = load_elems((const A*)acc, e0, cnt, vec);
#pragma unroll
    for (int j = 0; j < kEpl; j++) v.v[j] = v.v[j] / d;
    store_elems(acc, e0, cnt, vec, v);
  }
}

static int entry_grid(uint64_t nnz) {
  uint64_t blocks = (nnz + kBlock - 1) / kBlock;
  if (blocks > (uint64_t)kMaxBlocks * 4) blocks = (uint64_t)kMaxBlocks * 4;
  return (int)blocks;
}

static int check_type_n(int t, uint64_t n, const char* what) {
  return check_float_n(t, n, 31, what, " (the flat index is int32)");
}

// index, data and the flag record of a payload of nnz entries over n elements
static int check_payload(const void* index, const void* data, uintptr_t esz, uint64_t nnz, uint64_t n,
                         const void* flag, const char* what) {
  if (nnz > n) {
    sa_set_error("%s: more entries than the tensor has elements", what);
    return SA_ERR_ARG;
  }
  if (!flag || misaligned(flag, 4) || (nnz && (!index || !data || misaligned(index, 4) || misaligned(data, esz)))) {
    sa_set_error("%s: bad arguments (index, data and flag are required; element-aligned vectors)", what);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

}  // namespace coo
}  // namespace sa

using namespace sa::coo;

extern "C" int sa_coo_scratch_bytes(uint64_t n, int x_type) {
  const int rc = check_type_n(x_type, n, "sa_coo_scratch_bytes");
  return rc == SA_OK ? (int)kScratchBytes : rc;
}

extern "C" int sa_coo_count(const void* x, int x_type, uint64_t n, void* scratch, void* nnz_out, void* stream) {
  const int rc = check_type_n(x_type, n, "sa_coo_count");
  if (rc != SA_OK) return rc;
  if ((n && !x) || misaligned(x, elem_size(x_type)) || !scratch || misaligned(scratch, 4) || !nnz_out ||
      misaligned(nnz_out, 4)) {
    sa_set_error("sa_coo_count: bad arguments (x, scratch and nnz_out are required; element-aligned x, "
                 "4-byte aligned scratch and nnz_out)");
    return SA_ERR_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  const Grid g = wave_grid(n, (uintptr_t)x);
  uint32_t* cnt = (uint32_t*)scratch;
  dispatch_float(x_type, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL(k_count<T>, dim3(g.grid), dim3(kBlock), 0, s, (const T*)x, n, g.len, g.vec, cnt);
  });
  SA_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_offsets, dim3(1), dim3(kBlock), 0, s, cnt, g.nwaves, (uint32_t*)nnz_out);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_coo_fill(const void* x, int x_type, uint64_t n, const void* scratch, void* index_out,
                           void* data_out, uint64_t cap, void* flag, void* stream) {
  const int rc = check_type_n(x_type, n, "sa_coo_fill");
  if (rc != SA_OK) return rc;
  const uintptr_t esz = elem_size(x_type);
  if (cap > n) {
    sa_set_error("sa_coo_fill: cap exceeds n");
    return SA_ERR_ARG;
  }
  if ((n && !x) || misaligned(x, esz) || !scratch || misaligned(scratch, 4) || !flag || misaligned(flag, 4) ||
      (cap && (!index_out || !data_out)) || misaligned(index_out, 4) || misaligned(data_out, esz)) {
    sa_set_error("sa_coo_fill: bad arguments (x, scratch, flag and, for cap > 0, index_out and data_out are "
                 "required; element-aligned vectors)");
    return SA_ERR_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  const Grid g = wave_grid(n, (uintptr_t)x);
  dispatch_float(x_type, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL(k_fill<T>, dim3(g.grid), dim3(kBlock), 0, s, (const T*)x, n, g.len, g.vec,
                       (const uint32_t*)scratch, (int32_t*)index_out, (T*)data_out, (uint32_t)cap, (uint32_t*)flag);
  });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_coo_decode(const void* index, const void* data, int x_type, uint64_t nnz, uint64_t n,
                             void* dense_out, void* flag, void* stream) {
  int rc = check_type_n(x_type, n, "sa_coo_decode");
  const uintptr_t esz = elem_size(x_type);
  if (rc == SA_OK) rc = check_payload(index, data, esz, nnz, n, flag, "sa_coo_decode");
  if (rc != SA_OK) return rc;
  if ((n && !dense_out) || misaligned(dense_out, esz)) {
    sa_set_error("sa_coo_decode: dense_out is required and element-aligned");
    return SA_ERR_ARG;
  }
  if (n == 0) return SA_OK;
  hipStream_t s = (hipStream_t)stream;
  SA_HIP_CHECK(hipMemsetAsync(dense_out, 0, n * esz, s));
  if (nnz == 0) return SA_OK;
  dispatch_float(x_type, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL(k_scatter<T>, dim3(entry_grid(nnz)), dim3(kBlock), 0, s, (const int32_t*)index,
                       (const T*)data, nnz, (uint32_t)n, (T*)dense_out, (uint32_t*)flag);
  });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_coo_axpy(const void* index, const void* data, int x_type, uint64_t nnz, double w, void* acc,
                           int acc_type, uint64_t n, void* flag, void* stream) {
  int rc = check_float(x_type, "sa_coo_axpy");
  if (rc == SA_OK) rc = check_type_n(acc_type, n, "sa_coo_axpy");
  if (rc != SA_OK) return rc;
  if (x_type == SA_F64 && acc_type == SA_F32) {
    sa_set_error("sa_coo_axpy: float64 data needs a float64 accumulator");
    return SA_ERR_ARG;
  }
  rc = check_payload(index, data, elem_size(x_type), nnz, n, flag, "sa_coo_axpy");
  if (rc != SA_OK) return rc;
  if ((n && !acc) || misaligned(acc, elem_size(acc_type))) {
    sa_set_error("sa_coo_axpy: acc is required and element-aligned");
    return SA_ERR_ARG;
  }
  if (nnz == 0) return SA_OK;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(entry_grid(nnz)), block(kBlock);
  const int32_t* idx = (const int32_t*)index;
  uint32_t* f = (uint32_t*)flag;
  // (data, accumulator): three pairs, stated one by one
  if (x_type == SA_F32 && acc_type == SA_F32)
    hipLaunchKernelGGL((k_axpy<float, float>), grid, block, 0, s, idx, (const float*)data, nnz, (uint32_t)n, (float)w,
                       (float*)acc, f);
  else if (x_type == SA_F32)
    hipLaunchKernelGGL((k_axpy<float, double>), grid, block, 0, s, idx, (const float*)data, nnz, (uint32_t)n, w,
                       (double*)acc, f);
  else
    hipLaunchKernelGGL((k_axpy<double, double>), grid, block, 0, s, idx, (const double*)data, nnz, (uint32_t)n, w,
                       (double*)acc, f);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_coo_gather(const void* index, uint64_t nnz, const void* x, int x_type, uint64_t n, void* data_out,
                             void* flag, void* stream) {
  const int rc = check_type_n(x_type, n, "sa_coo_gather");
  if (rc != SA_OK) return rc;
  const uintptr_t esz = elem_size(x_type);
  if (nnz > n) {
    sa_set_error("sa_coo_gather: more entries than the tensor has elements");
    return SA_ERR_ARG;
  }
  if (!flag || misaligned(flag, 4) || (nnz && (!index || !x || !data_out)) || misaligned(index, 4) ||
      misaligned(x, esz) || misaligned(data_out, esz)) {
    sa_set_error("sa_coo_gather: bad arguments (flag and, for nnz > 0, index, x and data_out are required; "
                 "element-aligned vectors)");
    return SA_ERR_ARG;
  }
  if (nnz == 0) return SA_OK;
  const uintptr_t o = (uintptr_t)data_out, oe = o + nnz * esz;
  if ((o < (uintptr_t)x + n * esz && (uintptr_t)x < oe) || (o < (uintptr_t)index + nnz * 4 && (uintptr_t)index < oe) ||
      (o < (uintptr_t)flag + 8 && (uintptr_t)flag < oe)) {
    sa_set_error("sa_coo_gather: data_out may alias nothing");
    return SA_ERR_ARG;
  }
  dispatch_float(x_type, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL(k_gather<T>, dim3(entry_grid(nnz)), dim3(kBlock), 0, (hipStream_t)stream,
                       (const int32_t*)index, nnz, (const T*)x, (uint32_t)n, (T*)data_out, (uint32_t*)flag);
  });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_coo_finish(void* acc, int acc_type, uint64_t n, double divisor, void* stream) {
  const int rc = check_type_n(acc_type, n, "sa_coo_finish");
  if (rc != SA_OK) return rc;
  if ((n && !acc) || misaligned(acc, elem_size(acc_type))) {
    sa_set_error("sa_coo_finish: acc is required and element-aligned");
    return SA_ERR_ARG;
  }
  if (n == 0) return SA_OK;
  const Grid g = wave_grid(n, (uintptr_t)acc);
  dispatch_float(acc_type, [&](auto t) {
    typedef decltype(t) A;
    hipLaunchKernelGGL(k_divide<A>, dim3(g.grid), dim3(kBlock), 0, (hipStream_t)stream, (A*)acc, n, g.len, g.vec,
                       (A)divisor);
  });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}
