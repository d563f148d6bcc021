// sa_elems.h — a lane's four consecutive elements of a tile, for streaming
// kernels (sa_stc.hip, sa_scr.hip, sa_coo.hip; sa_quant.hip takes the vector
// types; all through sa_compress.h; sa_dp.hip, sa_dp_secure.hip and
// sa_server.hip take the vector types too): 16-byte loads and stores where the
// caller found every vector 16-byte aligned, element accesses with the same
// lane-to-element map otherwise.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sa {
namespace elems {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int kEpl = 4;           // consecutive elements per lane and tile
constexpr int kTile = 64 * kEpl;  // elements per wave and tile

template <class T>
struct Elems {
  T v[kEpl];
};

// the lane's elements [e0, e0 + cnt) of a tile (cnt in 0..4; the rest 0):
// 16-byte loads on the aligned full-tile path
template <class T>
__device__ __forceinline__ Elems<T> load_elems(const T* p, uint64_t e0, int cnt, bool vec) {
  Elems<T> r;
  if (vec && cnt == kEpl) {
    if constexpr (sizeof(T) == 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(p + e0);
      r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
    } else {
      const f64x2 t0 = *reinterpret_cast<const f64x2*>(p + e0);
      const f64x2 t1 = *reinterpret_cast<const f64x2*>(p + e0 + 2);
      r.v[0] = t0.x, r.v[1] = t0.y, r.v[2] = t1.x, r.v[3] = t1.y;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kEpl; j++) r.v[j] = j < cnt ? p[e0 + j] : T(0);
  }
  return r;
}

template <class T>
__device__ __forceinline__ void store_elems(T* p, uint64_t e0, int cnt, bool vec, const Elems<T>& r) {
  if (vec && cnt == kEpl) {
    if constexpr (sizeof(T) == 4) {
      f32x4 t;
      t.x = r.v[0], t.y = r.v[1], t.z = r.v[2], t.w = r.v[3];
      *reinterpret_cast<f32x4*>(p + e0) = t;
    } else {
      f64x2 t0, t1;
      t0.x = r.v[0], t0.y = r.v[1], t1.x = r.v[2], t1.y = r.v[3];
      *reinterpret_cast<f64x2*>(p + e0) = t0;
      *reinterpret_cast<f64x2*>(p + e0 + 2) = t1;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kEpl; j++)
      if (j < cnt) p[e0 + j] = r.v[j];
  }
}

// how many of the lane's elements [e0, e0 + 4) lie below hi
__device__ __forceinline__ int lane_count(uint64_t e0, uint64_t hi) {
  return e0 >= hi ? 0 : (hi - e0 < (uint64_t)kEpl ? (int)(hi - e0) : kEpl);
}

}  // namespace elems
}  // namespace sa
