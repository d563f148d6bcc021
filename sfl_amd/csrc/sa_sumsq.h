// sa_sumsq.h — the clipping norm's first level, shared by sa_sumsq_f32
// (sa_dp.hip: the squares of a vector) and sa_smp_sumsq_f32 (sa_smp.hip: the
// squares of FedSMP's masked, scaled update, formed in registers).  What a
// lane squares comes from a loader; the grid, the lane-to-element map and the
// order of every addition are written once, here, so the two entries give
// the same bits for the same values.
//
// A loader L has
//   typedef ... Raw;                       what a lane fetches for 4 elements
//   Raw fetch(uint64_t i) const;           the loads of vector index i (elements 4i .. 4i + 3)
//   f32x4 value(const Raw&, uint64_t i) const;   the 4 float32 values to square
//   float one(uint64_t e) const;           element e alone (the n % 4 tail)
// fetch and value are separate so that every load of an unrolled step is
// issued before the first value is formed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sfl_sa.h"
#include "sa_elems.h"

namespace sa {

constexpr int kSumsqUnroll = 2;

__device__ __forceinline__ double sq4(elems::f32x4 v) {
  return (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
}

__device__ __forceinline__ double block_sum256(double acc) {
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  __shared__ double w[4];
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = acc;
  __syncthreads();
  return (w[0] + w[1]) + (w[2] + w[3]);
}

// the plain loader: x itself
struct SumsqVector {
  const float* x;
  typedef elems::f32x4 Raw;
  __device__ __forceinline__ Raw fetch(uint64_t i) const {
    return __builtin_nontemporal_load(reinterpret_cast<const elems::f32x4*>(x) + i);
  }
  __device__ __forceinline__ elems::f32x4 value(const Raw& r, uint64_t) const { return r; }
  __device__ __forceinline__ float one(uint64_t e) const { return x[e]; }
};

// per-block partial sums of the loader's squares in fp64 -> partials[blockIdx.x]
// (bdim: the kernel's blockDim.x, read in the kernel itself)
template <class L>
__device__ __forceinline__ void sumsq_partial(const L& ld, uint64_t n, double* __restrict__ partials, uint32_t bdim) {
  double acc = 0.0;
  const uint64_t n4 = n / 4;
  const uint64_t stride = (uint64_t)gridDim.x * bdim;
  uint64_t i = (uint64_t)blockIdx.x * bdim + threadIdx.x;
  for (; i + (kSumsqUnroll - 1) * stride < n4; i += kSumsqUnroll * stride) {
    typename L::Raw v[kSumsqUnroll];
#pragma unroll
    for (int u = 0; u < kSumsqUnroll; u++) v[u] = ld.fetch(i + u * stride);
#pragma unroll
    for (int u = 0; u < kSumsqUnroll; u++) acc += sq4(ld.value(v[u], i + u * stride));
  }
  for (; i < n4; i += stride) acc += sq4(ld.value(ld.fetch(i), i));
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const double v = ld.one(n4 * 4 + threadIdx.x);
    acc += v * v;
  }
  const double b = block_sum256(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = b;
}

// the grid depends on n only (not on the device's occupancy): the same
// partials, so the same float64 sum, on every board
inline int sumsq_grid(uint64_t n) {
  uint64_t want = (n / 4 + 255) / 256;
  if (want < 1) want = 1;
  return (int)(want < (uint64_t)SA_DP_PARTIALS ? want : (uint64_t)SA_DP_PARTIALS);
}

// sa_dp.hip: k_sumsq_final over `grid` partials, enqueued on `stream`
int launch_sumsq_final(const double* partials, int grid, double* sumsq, int accumulate, void* stream);

}  // namespace sa
