// sa_dp.hip — GaussianModelDP pre-step (sfl/security/privacy/mechanism/
// mechanism_fl.py:62-130): the clipping norm (deterministic two-level fp64
// reduction), the standalone clip+noise kernel, and sa_mask_dp, which runs
// the same clip+noise inside the single-client masking kernel.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/sfl_sa.h"
#include "pcg128.h"
#include "sa_elems.h"
#include "sa_internal.h"
#include "sa_philox.h"
#include "sa_sumsq.h"

namespace sa {

// per-block partial sums of x^2 in fp64 -> partials[blockIdx.x].  Two
// non-temporal 16-byte loads in flight per lane at a 1,024-block grid: the
// fastest of the forms tools/microbench/sumsq_rate.hip timed on MI355X
// (0.065 ms for 100M floats with the final step, 0.77 of HBM, where round
// 4's one load per lane took 0.077 ms; larger grids and a last-block fused
// final step -- whose device-wide fence costs ~45 us -- were slower).  The
// grid depends on n only, so the partials, and the float64 sum, are the
// same on every board and every run.
using elems::f32x4;

// the body is sa_sumsq.h's, with the loader that yields x[i]: sa_smp.hip runs
// the same body over FedSMP's update
__global__ void __launch_bounds__(256) k_sumsq_partial(const float* __restrict__ x, uint64_t n,
                                                       double* __restrict__ partials) {
  sumsq_partial(SumsqVector{x}, n, partials, blockDim.x);
}

// fixed-order sum of the partials (deterministic), then the layer's squared
// norm as the reference forms it (mechanism_fl.py:132-135 under numpy
// 1.23.5): np.linalg.norm of a float32 array is sqrt(float32 x.x) in
// float32; `** 2` of that float32 scalar with a python int is a float64
// square (numpy 1.x promotes scalar-scalar operations without value-based
// casting), exact; python's sum adds the layers in float64 from 0 ->
// *out (or *out + sq)
__global__ void __launch_bounds__(256) k_sumsq_final(const double* __restrict__ partials, int k, double* out,
                                                     int accumulate) {
  double acc = 0.0;
  for (int j = threadIdx.x; j < k; j += 256) acc += partials[j];
  acc = block_sum256(acc);
  if (threadIdx.x == 0) {
    const float norm = sqrt_f32_rn((float)acc);        // np.linalg.norm: float32 dot, float32 sqrt
    const double sq = __dmul_rn((double)norm, norm);  // ** 2: float64, exact
    *out = accumulate ? __dadd_rn(*out, sq) : sq;
  }
}

struct DpArgs {
  const float* x;
  float* out;
  uint64_t n;
  const double* sumsq;
  const double* sumsq_layer;
  double clip;                   // python float (the clip divides in float64)
  float sigma, updates, inv;     // inv: exact_recip_pow2(updates) or 0
  uint64_t key, block0;
};

template <bool kPow2>
__device__ __forceinline__ f32x4 dp_apply4(f32x4 v, float scale, const Normal4& z, const DpArgs& a) {
  f32x4 o;
  o.x = dp_apply_t<kPow2>(v.x, scale, z.z[0], a.sigma, a.updates, a.inv);
  o.y = dp_apply_t<kPow2>(v.y, scale, z.z[1], a.sigma, a.updates, a.inv);
  o.z = dp_apply_t<kPow2>(v.z, scale, z.z[2], a.sigma, a.updates, a.inv);
  o.w = dp_apply_t<kPow2>(v.w, scale, z.z[3], a.sigma, a.updates, a.inv);
  return o;
}

// x' = x * scale + N(0, sigma^2) / updates, 4 elements (one Philox block)
// per 16-byte non-temporal load and store, the loads issued before the noise
// is formed.  No grid stride: a workgroup owns T * 256 consecutive Philox
// blocks, lane t blocks t, t + 256, ..., and the grid is
// ceil(blocks / (256 T)), so every workgroup streams once and retires (the
// streaming shape that reached 0.77 of HBM for a copy,
// profiles/r05/stream_rate.jsonl "tile").  The product's T is 1: at 100M
// 0.142-0.144 ms (0.70 of HBM), against 0.148 ms for T = 2, 0.157 for 4 and
// 0.171-0.174 ms for an occupancy-sized grid-stride loop
// (profiles/r05/dp_tile_ab.txt).  In that loop, more than one block in
// flight per lane, plain instead of non-temporal accesses and a grid of 2x
// or 4x the occupancy lost as well (profiles/r05/dp_unroll_ab.txt,
// dp_forms_ab.txt).  The loops over T stay although each runs once: written
// without them the kernel has the same instructions in other registers, and
// this form is the one that was measured.
constexpr int kDpTile = 1;

template <bool kPow2, int T>
__device__ __forceinline__ void dp_perturb_tile(const DpArgs& a) {
  const float scale = dp_scale(a.sumsq, a.sumsq_layer, a.clip);
  const uint64_t nb = (a.n + 3) / 4;
  const uint64_t full = a.n / 4;  // blocks with 4 elements
  const f32x4* x4 = reinterpret_cast<const f32x4*>(a.x);
  f32x4* o4 = reinterpret_cast<f32x4*>(a.out);
  const uint64_t b0 = (uint64_t)blockIdx.x * (256 * T) + threadIdx.x;
  if (b0 + (uint64_t)(T - 1) * 256 < full) {
    f32x4 v[T];
#pragma unroll
    for (int u = 0; u < T; u++) v[u] = __builtin_nontemporal_load(x4 + b0 + u * 256);
    // keep every load ahead of the noise (the scheduler otherwise sinks it
    // below the Philox rounds)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < T; u++) {
      const Normal4 z = gauss4(a.key, a.block0 + b0 + u * 256);
      __builtin_nontemporal_store(dp_apply4<kPow2>(v[u], scale, z, a), o4 + b0 + u * 256);
    }
    return;
  }
  for (int u = 0; u < T; u++) {
    const uint64_t b = b0 + (uint64_t)u * 256;
    if (b >= nb) break;
    const Normal4 z = gauss4(a.key, a.block0 + b);
    if (b < full) {
      o4[b] = dp_apply4<kPow2>(x4[b], scale, z, a);
    } else {
      const uint64_t e = b * 4;
      for (int k = 0; e + k < a.n; k++)
        a.out[e + k] = dp_apply_t<kPow2>(a.x[e + k], scale, z.z[k], a.sigma, a.updates, a.inv);
    }
  }
}

__global__ void __launch_bounds__(256) k_dp_perturb(const DpArgs a) {
  if (a.inv != 0.0f)  // uniform: num_updates a power of two, multiply by its exact reciprocal
    dp_perturb_tile<true, kDpTile>(a);
  else
    dp_perturb_tile<false, kDpTile>(a);
}

}  // namespace sa

using namespace sa;

int sa::launch_sumsq_final(const double* partials, int grid, double* sumsq, int accumulate, void* stream) {
  hipLaunchKernelGGL(k_sumsq_final, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, grid, sumsq, accumulate);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

static bool dp_ok(const sa_dp* dp, const char* who) {
  if (dp_fields_ok(dp)) return true;
  sa_set_error("%s: bad sa_dp (sumsq set, num_updates > 0, counter0 %% 4 == 0 required)", who);
  return false;
}

extern "C" int sa_sumsq_f32(const float* x, uint64_t n, double* partials, double* sumsq, int accumulate,
                            void* stream) {
  if ((n > 0 && !x) || !partials || !sumsq || !aligned16(x)) {  // n == 0: x unread, *sumsq (+)= 0
    sa_set_error("sa_sumsq_f32: bad arguments (x must be 16-byte aligned)");
    return SA_ERR_ARG;
  }
  const int grid = sumsq_grid(n);
  hipLaunchKernelGGL(k_sumsq_partial, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, n, partials);
  SA_HIP_CHECK(hipGetLastError());
  return launch_sumsq_final(partials, grid, sumsq, accumulate, stream);
}

extern "C" int sa_dp_perturb_f32(const float* x, uint64_t n, const sa_dp* dp, float* out, void* stream) {
  if ((n > 0 && (!x || !out)) || !aligned16(x) || !aligned16(out)) {
    sa_set_error("sa_dp_perturb_f32: bad arguments (16-byte aligned x and out required)");
    return SA_ERR_ARG;
  }
  if (!dp_ok(dp, "sa_dp_perturb_f32")) return SA_ERR_ARG;
  if (n == 0) return SA_OK;
  DpArgs a{x,  out, n, dp->sumsq, dp->sumsq_layer, dp->l2_norm_clip, dp->noise_std, dp->num_updates,
           exact_recip_pow2(dp->num_updates), dp->key, dp->counter0 / 4};
  int grid;
  if (!tile_blocks(((n + 3) / 4 + kDpTile - 1) / kDpTile, &grid)) {
    sa_set_error("sa_dp_perturb_f32: n too large for the tile grid");
    return SA_ERR_ARG;
  }
  hipLaunchKernelGGL(k_dp_perturb, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_mask_dp(const float* x, uint64_t n, double weight, int fxp_bits, const sa_mask_stream* streams,
                          int n_streams, const sa_dp* dp, uint64_t* out, uint64_t* sum_accum, uint64_t* digest,
                          uint32_t* flags, void* stream) {
  if (!x && n > 0) {
    sa_set_error("sa_mask_dp: x is required");
    return SA_ERR_ARG;
  }
  if (!dp_ok(dp, "sa_mask_dp")) return SA_ERR_ARG;
  return sa_mask_impl(x, SA_F32, SA_F32, n, weight, nullptr, fxp_bits, streams, n_streams, out, sum_accum, digest,
                      flags, stream, dp);
}
