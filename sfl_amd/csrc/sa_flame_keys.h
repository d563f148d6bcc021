// sa_flame_keys.h — what sa_flame.hip and sa_flame_wide.hip share: the packed
// layout of FlameAggregator's statistics and the integer keys by which the
// medians are ordered.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sa {
namespace flame {

__host__ __device__ constexpr int gram_count(int c) { return c * (c + 1) / 2; }
__host__ __device__ constexpr int stat_count(int c) { return gram_count(c) + c; }
// the slot of G[i][i] in the packed upper triangle (row-major, j >= i)
__host__ __device__ constexpr int row_slot(int c, int i) { return i * c - i * (i - 1) / 2; }

// --- the order: integer keys --------------------------------------------------
template <class T>
struct Key;
template <>
struct Key<float> {
  typedef int32_t type;
  static constexpr int32_t kMag = 0x7fffffff;
};
template <>
struct Key<double> {
  typedef int64_t type;
  static constexpr int64_t kMag = 0x7fffffffffffffffll;
};

// the bit pattern as a signed integer whose order is the values' order with
// -0 < +0 (negative patterns have their magnitude bits flipped); its own inverse
template <class T>
__device__ __forceinline__ typename Key<T>::type to_key(T x) {
  typedef typename Key<T>::type K;
  K b;
  __builtin_memcpy(&b, &x, sizeof b);
  return b ^ ((b >> (8 * (int)sizeof(K) - 1)) & Key<T>::kMag);
}
template <class T>
__device__ __forceinline__ T from_key(typename Key<T>::type k) {
  typedef typename Key<T>::type K;
  const K b = k ^ ((k >> (8 * (int)sizeof(K) - 1)) & Key<T>::kMag);
  T x;
  __builtin_memcpy(&x, &b, sizeof x);
  return x;
}

}  // namespace flame
}  // namespace sa
