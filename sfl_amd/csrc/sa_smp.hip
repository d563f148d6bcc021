// sa_smp.hip — FedSMP, sparsified model perturbation (examples/security/h_gia/
// FedSMP_defense/FedSMP_torch.py:105-119 on the worker, :193-201 the server's
// mask): a keyed Bernoulli mask regenerated in registers, the clipping norm of
// the masked, scaled update (sa_sumsq.h's body over a loader that forms the
// update), and the upload old + mask * (clip + noise)(mask * (new - old) / c)
// in one streaming pass.  The definition is in include/sfl_sa.h.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/sfl_sa.h"
#include "sa_elems.h"
#include "sa_internal.h"
#include "sa_philox.h"
#include "sa_sumsq.h"

namespace sa {
namespace smp {

using elems::f32x4;

// the four mask words of stream indices 4 blk .. 4 blk + 3: Philox4x32-10 on
// (lo32(blk), hi32(blk), 1, 0); the 1 keeps the mask's words apart from the DP
// noise's (philox_block: 0 there) under one key
SA_PHX_HD inline void mask_words(uint64_t key, uint64_t blk, uint32_t c[4]) {
  c[0] = (uint32_t)blk;
  c[1] = (uint32_t)(blk >> 32);
  c[2] = 1u;
  c[3] = 0u;
  philox4x32_10(c, (uint32_t)key, (uint32_t)(key >> 32));
}

struct Mask {
  uint64_t key, block0, threshold;  // block0: counter0 / 4
  float c;                          // the divisor, np.float32(p + 1e-6)
};

struct Kept4 {
  bool k[4];
};

__device__ __forceinline__ Kept4 kept4(const Mask& m, uint64_t b) {
  uint32_t w[4];
  mask_words(m.key, m.block0 + b, w);
  Kept4 r;
#pragma unroll
  for (int j = 0; j < 4; j++) r.k[j] = (uint64_t)w[j] < m.threshold;
  return r;
}

// d = kept ? (w1 - w0) / c : +0, every operation rounded in float32
__device__ __forceinline__ float delta1(float w0, float w1, bool kept, float c) {
  return kept ? __fdiv_rn(__fsub_rn(w1, w0), c) : 0.0f;
}

__device__ __forceinline__ f32x4 delta4(f32x4 a, f32x4 b, const Kept4& k, float c) {
  f32x4 d;
  d.x = delta1(a.x, b.x, k.k[0], c);
  d.y = delta1(a.y, b.y, k.k[1], c);
  d.z = delta1(a.z, b.z, k.k[2], c);
  d.w = delta1(a.w, b.w, k.k[3], c);
  return d;
}

// --- the clipping norm: sa_sumsq.h's body over d ----------------------------
struct SumsqDelta {
  const float* w0;
  const float* w1;
  Mask m;
  struct Raw {
    f32x4 a, b;
  };
  __device__ __forceinline__ Raw fetch(uint64_t i) const {
    return Raw{__builtin_nontemporal_load(reinterpret_cast<const f32x4*>(w0) + i),
               __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(w1) + i)};
  }
  __device__ __forceinline__ f32x4 value(const Raw& r, uint64_t i) const {
    return delta4(r.a, r.b, kept4(m, i), m.c);
  }
  __device__ __forceinline__ float one(uint64_t e) const {
    const Kept4 k = kept4(m, e >> 2);
    const int j = (int)(e & 3);
    return delta1(w0[e], w1[e], j == 0 ? k.k[0] : j == 1 ? k.k[1] : j == 2 ? k.k[2] : k.k[3], m.c);
  }
};

__global__ void __launch_bounds__(256) k_smp_sumsq_partial(const float* __restrict__ w0,
                                                           const float* __restrict__ w1, uint64_t n, const Mask m,
                                                           double* __restrict__ partials) {
  sumsq_partial(SumsqDelta{w0, w1, m}, n, partials, blockDim.x);
}

// --- the one-pass tile kernels ----------------------------------------------
// k_dp_perturb's measured shape (sa_dp.hip): one Philox block (4 elements)
// per lane, one tile of 256 blocks per workgroup, no grid stride,
// non-temporal 16-byte accesses, the loads issued before the Philox rounds.
// An Op says what becomes of a lane's elements:
//   Ctx prep(b)                      per-block state (the block's normals)
//   float one(a, s, kept, ctx, j)    element j of the block: a from w0, s from
//                                    the second vector (w1, or t for finish)
struct TileArgs {
  const float* w0;
  const float* second;  // w1 (delta, perturb) or t (finish); out may alias it
  float* out;
  uint64_t n;
  Mask m;
};

template <class Op>
__device__ __forceinline__ void smp_tile(const TileArgs& a, const Op& op) {
  const uint64_t nb = (a.n + 3) / 4;
  const uint64_t full = a.n / 4;  // blocks with 4 elements
  const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b < full) {
    const f32x4 x = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.w0) + b);
    const f32x4 s = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.second) + b);
    // keep both loads ahead of the Philox rounds
    __builtin_amdgcn_sched_barrier(0);
    const Kept4 k = kept4(a.m, b);
    const typename Op::Ctx ctx = op.prep(b);
    f32x4 o;
    o.x = op.one(x.x, s.x, k.k[0], ctx, 0);
    o.y = op.one(x.y, s.y, k.k[1], ctx, 1);
    o.z = op.one(x.z, s.z, k.k[2], ctx, 2);
    o.w = op.one(x.w, s.w, k.k[3], ctx, 3);
    __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(a.out) + b);
    return;
  }
  if (b >= nb) return;
  const Kept4 k = kept4(a.m, b);
  const typename Op::Ctx ctx = op.prep(b);
  const uint64_t e = b * 4;
  // constant indices (a runtime j would move k and ctx into LDS)
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (e + j < a.n) a.out[e + j] = op.one(a.w0[e + j], a.second[e + j], k.k[j], ctx, j);
}

struct NoCtx {};

// d, materialised
struct OpDelta {
  float c;
  typedef NoCtx Ctx;
  __device__ __forceinline__ Ctx prep(uint64_t) const { return Ctx{}; }
  __device__ __forceinline__ float one(float a, float s, bool kept, const Ctx&, int) const {
    return delta1(a, s, kept, c);
  }
};

// kept ? w0 + t : w0
struct OpFinish {
  typedef NoCtx Ctx;
  __device__ __forceinline__ Ctx prep(uint64_t) const { return Ctx{}; }
  __device__ __forceinline__ float one(float a, float s, bool kept, const Ctx&, int) const {
    return kept ? __fadd_rn(a, s) : a;
  }
};

// kept ? w0 + d : w0 (no model_gdp)
struct OpPlain {
  float c;
  typedef NoCtx Ctx;
  __device__ __forceinline__ Ctx prep(uint64_t) const { return Ctx{}; }
  __device__ __forceinline__ float one(float a, float s, bool kept, const Ctx&, int) const {
    return kept ? __fadd_rn(a, delta1(a, s, true, c)) : a;
  }
};

// kept ? w0 + (d scale + (z sigma) / num_updates) : w0, dp_apply_t on d
struct DpPart {
  const double* sumsq;
  const double* sumsq_layer;
  double clip;
  float sigma, updates, inv;
  uint64_t key, block0;
};

template <bool kPow2>
struct OpPerturb {
  float c, scale;
  DpPart d;
  typedef Normal4 Ctx;
  __device__ __forceinline__ Ctx prep(uint64_t b) const { return gauss4(d.key, d.block0 + b); }
  __device__ __forceinline__ float one(float a, float s, bool kept, const Ctx& z, int j) const {
    const float t = dp_apply_t<kPow2>(delta1(a, s, true, c), scale, z.z[j], d.sigma, d.updates, d.inv);
    return kept ? __fadd_rn(a, t) : a;
  }
};

__global__ void __launch_bounds__(256) k_smp_delta(const TileArgs a) { smp_tile(a, OpDelta{a.m.c}); }
__global__ void __launch_bounds__(256) k_smp_finish(const TileArgs a) { smp_tile(a, OpFinish{}); }
__global__ void __launch_bounds__(256) k_smp_plain(const TileArgs a) { smp_tile(a, OpPlain{a.m.c}); }
__global__ void __launch_bounds__(256) k_smp_perturb(const TileArgs a, const DpPart d) {
  const float scale = dp_scale(d.sumsq, d.sumsq_layer, d.clip);
  if (d.inv != 0.0f)  // uniform: num_updates a power of two, multiply by its exact reciprocal
    smp_tile(a, OpPerturb<true>{a.m.c, scale, d});
  else
    smp_tile(a, OpPerturb<false>{a.m.c, scale, d});
}

// the mask as bytes: one Philox block, 4 bytes, per lane
__global__ void __launch_bounds__(256) k_smp_mask(const Mask m, uint64_t n, int vec, uint8_t* __restrict__ out) {
  const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= (n + 3) / 4) return;
  const Kept4 k = kept4(m, b);
  const uint64_t e = b * 4;
  if (vec && e + 4 <= n) {
    *reinterpret_cast<uint32_t*>(out + e) =
        (uint32_t)k.k[0] | (uint32_t)k.k[1] << 8 | (uint32_t)k.k[2] << 16 | (uint32_t)k.k[3] << 24;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (e + j < n) out[e + j] = k.k[j];
  }
}

// --- entry checks -------------------------------------------------------------
static int check_smp(const sa_smp* smp, bool divides, const char* who) {
  if (!smp) {
    sa_set_error("%s: smp is required", who);
    return SA_ERR_ARG;
  }
  if (smp->counter0 & 3) {
    sa_set_error("%s: smp->counter0 must be a multiple of 4", who);
    return SA_ERR_ARG;
  }
  if (smp->threshold > (1ull << 32)) {
    sa_set_error("%s: smp->threshold exceeds 2^32", who);
    return SA_ERR_ARG;
  }
  if (divides && !(smp->divisor > 0.0f)) {
    sa_set_error("%s: smp->divisor must be positive", who);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

// a float32 vector of a non-empty call: required and 16-byte aligned
static int check_vec(const void* p, const char* name, const char* who) {
  if (!p) {
    sa_set_error("%s: %s is required", who, name);
    return SA_ERR_ARG;
  }
  if (!aligned16(p)) {
    sa_set_error("%s: %s must be 16-byte aligned", who, name);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

static int check_grid(uint64_t n, int* grid, const char* who) {
  if (!tile_blocks(n / 4 + ((n & 3) != 0), grid)) {  // not (n + 3) / 4: it wraps at the top of uint64
    sa_set_error("%s: n too large for the tile grid", who);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

static Mask mask_of(const sa_smp* smp) { return Mask{smp->key, smp->counter0 / 4, smp->threshold, smp->divisor}; }

// the three entries that map (w0, second) -> out under the mask alone
template <class K>
static int launch_pair(K kernel, const float* w0, const float* second, const char* second_name, uint64_t n,
                       const sa_smp* smp, bool divides, float* out, void* stream, const char* who) {
  int rc = check_smp(smp, divides, who);
  if (rc != SA_OK || n == 0) return rc;
  if ((rc = check_vec(w0, "w0", who)) != SA_OK || (rc = check_vec(second, second_name, who)) != SA_OK ||
      (rc = check_vec(out, "out", who)) != SA_OK)
    return rc;
  int grid;
  if ((rc = check_grid(n, &grid, who)) != SA_OK) return rc;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, TileArgs{w0, second, out, n, mask_of(smp)});
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

}  // namespace smp
}  // namespace sa

using namespace sa;
using namespace sa::smp;

extern "C" int sa_smp_mask_host(const sa_smp* smp, uint64_t n, uint8_t* out) {
  const int rc = check_smp(smp, false, "sa_smp_mask_host");
  if (rc != SA_OK || n == 0) return rc;
  if (!out) {
    sa_set_error("sa_smp_mask_host: out is required");
    return SA_ERR_ARG;
  }
  const Mask m = mask_of(smp);
  for (uint64_t b = 0; 4 * b < n; b++) {
    uint32_t w[4];
    mask_words(m.key, m.block0 + b, w);
    for (int j = 0; j < 4 && 4 * b + j < n; j++) out[4 * b + j] = (uint64_t)w[j] < m.threshold;
  }
  return SA_OK;
}

extern "C" int sa_smp_mask(const sa_smp* smp, uint64_t n, uint8_t* out, void* stream) {
  int rc = check_smp(smp, false, "sa_smp_mask");
  if (rc != SA_OK || n == 0) return rc;
  if (!out) {
    sa_set_error("sa_smp_mask: out is required");
    return SA_ERR_ARG;
  }
  int grid;
  if ((rc = check_grid(n, &grid, "sa_smp_mask")) != SA_OK) return rc;
  hipLaunchKernelGGL(k_smp_mask, dim3(grid), dim3(256), 0, (hipStream_t)stream, mask_of(smp), n,
                     (int)(((uintptr_t)out & 3) == 0), out);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_smp_delta_f32(const float* w0, const float* w1, uint64_t n, const sa_smp* smp, float* out,
                                void* stream) {
  return launch_pair(k_smp_delta, w0, w1, "w1", n, smp, true, out, stream, "sa_smp_delta_f32");
}

extern "C" int sa_smp_finish_f32(const float* w0, const float* t, uint64_t n, const sa_smp* smp, float* out,
                                 void* stream) {
  return launch_pair(k_smp_finish, w0, t, "t", n, smp, false, out, stream, "sa_smp_finish_f32");
}

extern "C" int sa_smp_sumsq_f32(const float* w0, const float* w1, uint64_t n, const sa_smp* smp, double* partials,
                                double* sumsq, int accumulate, void* stream) {
  const char* who = "sa_smp_sumsq_f32";
  int rc = check_smp(smp, true, who);
  if (rc != SA_OK) return rc;
  if (!partials || !sumsq) {  // as sa_sumsq_f32: n == 0 still stores (or adds) 0
    sa_set_error("%s: %s is required", who, partials ? "sumsq" : "partials");
    return SA_ERR_ARG;
  }
  if (n > 0 && ((rc = check_vec(w0, "w0", who)) != SA_OK || (rc = check_vec(w1, "w1", who)) != SA_OK)) return rc;
  int tiles;
  if ((rc = check_grid(n, &tiles, who)) != SA_OK) return rc;
  const int grid = sumsq_grid(n);
  hipLaunchKernelGGL(k_smp_sumsq_partial, dim3(grid), dim3(256), 0, (hipStream_t)stream, w0, w1, n, mask_of(smp),
                     partials);
  SA_HIP_CHECK(hipGetLastError());
  return launch_sumsq_final(partials, grid, sumsq, accumulate, stream);
}

extern "C" int sa_smp_perturb_f32(const float* w0, const float* w1, uint64_t n, const sa_smp* smp, const sa_dp* dp,
                                  float* out, void* stream) {
  const char* who = "sa_smp_perturb_f32";
  if (!dp) return launch_pair(k_smp_plain, w0, w1, "w1", n, smp, true, out, stream, who);
  int rc = check_smp(smp, true, who);
  if (rc != SA_OK) return rc;
  if (!dp_fields_ok(dp)) {
    sa_set_error("%s: bad sa_dp (sumsq set, num_updates > 0, counter0 %% 4 == 0 required)", who);
    return SA_ERR_ARG;
  }
  if (n == 0) return SA_OK;
  if ((rc = check_vec(w0, "w0", who)) != SA_OK || (rc = check_vec(w1, "w1", who)) != SA_OK ||
      (rc = check_vec(out, "out", who)) != SA_OK)
    return rc;
  int grid;
  if ((rc = check_grid(n, &grid, who)) != SA_OK) return rc;
  const DpPart d{dp->sumsq, dp->sumsq_layer, dp->l2_norm_clip, dp->noise_std, dp->num_updates,
                 exact_recip_pow2(dp->num_updates), dp->key, dp->counter0 / 4};
  hipLaunchKernelGGL(k_smp_perturb, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                     TileArgs{w0, w1, out, n, mask_of(smp)}, d);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}
