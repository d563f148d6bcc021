// sa_dp_secure.hip — GaussianModelDP with is_secure_generator
// (mechanism_fl.py:112-127 over sfl/security/random/distrbutions.py:89-137):
// the clip of sa_dp.hip, the noise from a ChaCha20 keystream and the
// Holohan-Braghin transform in float64 (sa_chacha.h; the contract is in
// include/sfl_sa.h).  Also the raw keystream and the transform alone, which
// make the two halves testable bit for bit.
#include <hip/hip_runtime.h>

#include "../../include/sfl_sa.h"
#include "sa_elems.h"
#include "sa_internal.h"
#include "sa_philox.h"
#include "sa_chacha.h"

namespace sa {

using elems::f32x4;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct ChachaKey {
  uint32_t k[8];
};

struct DpSecureArgs {
  const float* x;
  float* out;
  uint64_t n;
  const double* sumsq;
  const double* sumsq_layer;
  double clip, sigma;
  float updates;
  ChachaKey key;
  uint64_t nonce, block0;
};

// x' = fl32(x * scale) + fl32((float)z64 / updates): mechanism_fl.py:112-127
// (clip, astype(float32) noise, noise / num_updates, np.add)
__device__ __forceinline__ float dp_secure_apply(float x, float scale, double z64, float updates) {
  return __fadd_rn(__fmul_rn(x, scale), __fdiv_rn((float)z64, updates));
}

// The tile form of k_dp_perturb (sa_dp.hip): one ChaCha block = 4 elements =
// one 16-byte non-temporal load and store per lane, 256 blocks per
// workgroup, no grid stride; the load is issued before the rounds.  The
// kernel is issue-bound (20 rounds and four float64 log / sin / cos per
// lane), far below HBM: DESIGN.md section 4.
__global__ void __launch_bounds__(256) k_dp_perturb_secure(const DpSecureArgs a) {
  const uint64_t nb = (a.n + 3) / 4;
  const uint64_t full = a.n / 4;  // blocks with 4 elements
  const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= nb) return;
  const float scale = dp_scale(a.sumsq, a.sumsq_layer, a.clip);
  const f32x4* x4 = reinterpret_cast<const f32x4*>(a.x);
  f32x4* o4 = reinterpret_cast<f32x4*>(a.out);
  uint32_t o[16];
  if (b < full) {
    const f32x4 v = __builtin_nontemporal_load(x4 + b);
    __builtin_amdgcn_sched_barrier(0);
    chacha20_block(a.key.k, a.nonce, a.block0 + b, o);
    f32x4 y;
    y.x = dp_secure_apply(v.x, scale, hb_normal(o[0], o[1], o[2], o[3], a.sigma), a.updates);
    y.y = dp_secure_apply(v.y, scale, hb_normal(o[4], o[5], o[6], o[7], a.sigma), a.updates);
    y.z = dp_secure_apply(v.z, scale, hb_normal(o[8], o[9], o[10], o[11], a.sigma), a.updates);
    y.w = dp_secure_apply(v.w, scale, hb_normal(o[12], o[13], o[14], o[15], a.sigma), a.updates);
    __builtin_nontemporal_store(y, o4 + b);
    return;
  }
  // the last, partial block: 1..3 elements
  chacha20_block(a.key.k, a.nonce, a.block0 + b, o);
  const uint64_t e = b * 4;
  for (int k = 0; k < 3 && e + k < a.n; k++)
    a.out[e + k] = dp_secure_apply(a.x[e + k], scale, hb_normal(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3],
                                                              a.sigma), a.updates);
}

// the raw keystream: one block (four 16-byte stores) per lane
__global__ void __launch_bounds__(256) k_chacha20_keystream(const ChachaKey key, uint64_t nonce, uint64_t block0,
                                                            uint64_t n_blocks, uint32_t* __restrict__ out) {
  const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= n_blocks) return;
  uint32_t o[16];
  chacha20_block(key.k, nonce, block0 + b, o);
  u32x4* o4 = reinterpret_cast<u32x4*>(out) + b * 4;
#pragma unroll
  for (int q = 0; q < 4; q++) o4[q] = u32x4{o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]};
}

// the transform alone: one normal per lane from four words
__global__ void __launch_bounds__(256) k_hb_normals(const uint32_t* __restrict__ words, uint64_t n, double sigma,
                                                    double* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t* w = words + 4 * i;
  out[i] = hb_normal(w[0], w[1], w[2], w[3], sigma);
}

static bool tile_grid(uint64_t items, const char* who, int* grid) {
  if (tile_blocks(items, grid)) return true;
  sa_set_error("%s: too many elements for the tile grid", who);
  return false;
}

}  // namespace sa

using namespace sa;

extern "C" int sa_dp_perturb_secure_f32(const float* x, uint64_t n, const sa_dp_secure* dp, float* out,
                                        void* stream) {
  if ((n > 0 && (!x || !out)) || !aligned16(x) || !aligned16(out)) {
    sa_set_error("sa_dp_perturb_secure_f32: bad arguments (16-byte aligned x and out required)");
    return SA_ERR_ARG;
  }
  if (!dp_fields_ok(dp)) {
    sa_set_error("sa_dp_perturb_secure_f32: bad sa_dp_secure (sumsq set, num_updates > 0, counter0 %% 4 == 0 "
                 "required)");
    return SA_ERR_ARG;
  }
  if (n == 0) return SA_OK;
  int grid;
  if (!tile_grid((n + 3) / 4, "sa_dp_perturb_secure_f32", &grid)) return SA_ERR_ARG;
  DpSecureArgs a{x, out, n, dp->sumsq, dp->sumsq_layer, dp->l2_norm_clip, dp->noise_std, dp->num_updates,
                 {}, dp->nonce, dp->counter0 / 4};
  for (int i = 0; i < 8; i++) a.key.k[i] = dp->key[i];
  hipLaunchKernelGGL(k_dp_perturb_secure, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_chacha20_keystream(const uint32_t key[8], uint64_t nonce, uint64_t block0, uint64_t n_blocks,
                                     uint32_t* out, void* stream) {
  if (!key || (n_blocks > 0 && !out) || !aligned16(out)) {
    sa_set_error("sa_chacha20_keystream: bad arguments (key and a 16-byte aligned out required)");
    return SA_ERR_ARG;
  }
  if (n_blocks == 0) return SA_OK;
  int grid;
  if (!tile_grid(n_blocks, "sa_chacha20_keystream", &grid)) return SA_ERR_ARG;
  ChachaKey k;
  for (int i = 0; i < 8; i++) k.k[i] = key[i];
  hipLaunchKernelGGL(k_chacha20_keystream, dim3(grid), dim3(256), 0, (hipStream_t)stream, k, nonce, block0, n_blocks,
                     out);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_hb_normals_f64(const uint32_t* words, uint64_t n, double sigma, double* out, void* stream) {
  if (n > 0 && (!words || !out)) {
    sa_set_error("sa_hb_normals_f64: bad arguments (words and out required)");
    return SA_ERR_ARG;
  }
  if (n == 0) return SA_OK;
  int grid;
  if (!tile_grid(n, "sa_hb_normals_f64", &grid)) return SA_ERR_ARG;
  hipLaunchKernelGGL(k_hb_normals, dim3(grid), dim3(256), 0, (hipStream_t)stream, words, n, sigma, out);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}
