// sa_runs.h — the lane-run layout of the streaming code passes (sa_quant.hip,
// sa_kmeans.hip; nothing else includes it): a lane owns a run of consecutive
// elements whose codes leave or arrive in one 16-byte access, behind a scalar
// head that brings the code pointer to its vector's alignment and before a
// scalar tail.  sa_quant.hip's head comment has the layout and what it was
// measured against.
#pragma once
#include <hip/hip_runtime.h>

#include "sa_compress.h"

namespace sa {
namespace runs {

using namespace sa::entry;
using sa::elems::f32x4;
using sa::elems::f64x2;
using sa::wave::kBlock;

// the grid's bound: 2 resident blocks per CU on 256 CUs.  Measured at 100M
// elements against 256, 1024 and 2048: the passes that
// HBM bounds are fastest here
constexpr int kMaxBlocks = 512;
constexpr int kEncRun = 16;  // elements per lane and run, encoding: one 16-byte store of int8 codes
template <class T>
constexpr int kDecRun = 16 / sizeof(T);  // decoding: one 16-byte store of floats

// kCount consecutive T at p: 16-byte accesses if `vec`, element accesses otherwise
template <class T, int kCount>
__device__ __forceinline__ void load_run(const T* __restrict__ p, T* v, bool vec) {
  if (vec) {
    if constexpr (sizeof(T) == 4) {
#pragma unroll
      for (int k = 0; k < kCount / 4; k++) {
        const f32x4 t = reinterpret_cast<const f32x4*>(p)[k];
        v[4 * k] = t.x, v[4 * k + 1] = t.y, v[4 * k + 2] = t.z, v[4 * k + 3] = t.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < kCount / 2; k++) {
        const f64x2 t = reinterpret_cast<const f64x2*>(p)[k];
        v[2 * k] = t.x, v[2 * k + 1] = t.y;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < kCount; j++) v[j] = p[j];
  }
}

template <class T, int kCount>
__device__ __forceinline__ void store_run(T* __restrict__ p, const T* v, bool vec) {
  if (vec) {
    if constexpr (sizeof(T) == 4) {
#pragma unroll
      for (int k = 0; k < kCount / 4; k++) {
        f32x4 t;
        t.x = v[4 * k], t.y = v[4 * k + 1], t.z = v[4 * k + 2], t.w = v[4 * k + 3];
        reinterpret_cast<f32x4*>(p)[k] = t;
      }
    } else {
#pragma unroll
      for (int k = 0; k < kCount / 2; k++) {
        f64x2 t;
        t.x = v[2 * k], t.y = v[2 * k + 1];
        reinterpret_cast<f64x2*>(p)[k] = t;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < kCount; j++) p[j] = v[j];
  }
}

// the codes of a run of RUN elements, RUN * QB bytes (2 .. 32), in words
// (little-endian, element order)
template <int QB, int RUN>
struct Codes {
  static constexpr int kBytes = RUN * QB;
  static constexpr int kWords = kBytes < 4 ? 1 : kBytes / 4;
  static constexpr int kPerWord = 4 / QB;
  static constexpr uintptr_t kAlign = kBytes > 16 ? 16 : kBytes;  // of the vector access
  uint32_t w[kWords];

  __device__ __forceinline__ void pack(const int32_t* c) {
#pragma unroll
    for (int k = 0; k < kWords; k++) w[k] = 0;
#pragma unroll
    for (int i = 0; i < RUN; i++)
      w[i / kPerWord] |= ((uint32_t)c[i] & (QB == 1 ? 0xffu : 0xffffu)) << (8 * QB * (i % kPerWord));
  }
  __device__ __forceinline__ void unpack(int32_t* c) const {
#pragma unroll
    for (int i = 0; i < RUN; i++) {
      const uint32_t f = w[i / kPerWord] >> (8 * QB * (i % kPerWord));
      c[i] = QB == 1 ? (int32_t)(int8_t)(f & 0xffu) : (int32_t)(int16_t)(f & 0xffffu);
    }
  }
  // p is kAlign-aligned; a store is at least 4 bytes
  __device__ __forceinline__ void store(void* __restrict__ p) const {
    static_assert(kBytes >= 4, "the codes leave in stores of at least 4 bytes");
    if constexpr (kWords == 1) {
      *reinterpret_cast<uint32_t*>(p) = w[0];
    } else if constexpr (kWords == 2) {
      *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
    } else {
#pragma unroll
      for (int k = 0; k < kWords / 4; k++)
        reinterpret_cast<uint4*>(p)[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    }
  }
  __device__ __forceinline__ void load(const void* __restrict__ p) {
    if constexpr (kBytes == 2) {
      w[0] = *reinterpret_cast<const uint16_t*>(p);
    } else if constexpr (kWords == 1) {
      w[0] = *reinterpret_cast<const uint32_t*>(p);
    } else if constexpr (kWords == 2) {
      const uint2 t = *reinterpret_cast<const uint2*>(p);
      w[0] = t.x, w[1] = t.y;
    } else {
#pragma unroll
      for (int k = 0; k < kWords / 4; k++) {
        const uint4 t = reinterpret_cast<const uint4*>(p)[k];
        w[4 * k] = t.x, w[4 * k + 1] = t.y, w[4 * k + 2] = t.z, w[4 * k + 3] = t.w;
      }
    }
  }
};

template <int QB>
__device__ __forceinline__ void store_code(void* q, uint64_t i, int32_t c) {
  if constexpr (QB == 1)
    reinterpret_cast<int8_t*>(q)[i] = (int8_t)c;
  else
    reinterpret_cast<int16_t*>(q)[i] = (int16_t)c;
}
template <int QB>
__device__ __forceinline__ int32_t load_code(const void* q, uint64_t i) {
  if constexpr (QB == 1)
    return reinterpret_cast<const int8_t*>(q)[i];
  else
    return reinterpret_cast<const int16_t*>(q)[i];
}

// --- launch geometry and checks -----------------------------------------------

struct Plan {
  uint32_t head;
  uint64_t nruns;
  int vec, grid;
};

// `coarse`: the pointer the head aligns, to `align` bytes in steps of `step`;
// `fine`: the float vector, 16-byte accessed if aligned behind the head
static Plan plan_of(uint64_t n, const void* coarse, uintptr_t align, uintptr_t step, const void* fine, uintptr_t esz,
                    int run, int unroll, int max_blocks = kMaxBlocks) {
  Plan p;
  const uintptr_t off = (uintptr_t)coarse & (align - 1);
  uint64_t head = off ? (align - off) / step : 0;
  if (head > n) head = n;
  p.head = (uint32_t)head;
  p.nruns = (n - head) / run;
  p.vec = (((uintptr_t)fine + head * esz) & 15) == 0;
  uint64_t blocks = (p.nruns + (uint64_t)kBlock * unroll - 1) / ((uint64_t)kBlock * unroll);
  if (blocks > (uint64_t)max_blocks) blocks = max_blocks;
  if (blocks == 0) blocks = 1;
  p.grid = (int)blocks;
  return p;
}

// the float vector and the code vector of n elements
static int check_vectors(const void* x, uintptr_t esz, const void* q, int q_bytes, uint64_t n, const char* what) {
  if (q_bytes != 1 && q_bytes != 2) {
    sa_set_error("%s: q_bytes must be 1 (int8 codes) or 2 (int16 codes)", what);
    return SA_ERR_ARG;
  }
  if ((n && (!x || !q)) || misaligned(x, esz) || misaligned(q, (uintptr_t)q_bytes)) {
    sa_set_error("%s: bad arguments (the data and the codes are required; element-aligned vectors)", what);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

}  // namespace runs
}  // namespace sa
