// Microbenchmark: issue efficiency of the hand-scheduled PCG64 draw
// (sa_clients_impl.h, SA_PCG_DRAW_ASM) outside the product kernel.
// Question it answers: where do the ~40% between the tight-loop draw rate and
// the k_clients draw rate go — occupancy, LDS-resident constants, or the
// asm-volatile serialisation of one stream's chain?
// Standalone tool; not part of the product.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 draw_issue.hip -o draw_issue
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "../../sfl_amd/csrc/sa_clients_impl.h"

#define CHECK(x)                                                                                      \
  do {                                                                                                \
    hipError_t e_ = (x);                                                                              \
    if (e_ != hipSuccess) {                                                                           \
      fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__);          \
      return 1;                                                                                       \
    }                                                                                                 \
  } while (0)

using namespace sa;

struct StreamLds {
  uint64_t inc_lo, inc_hi, cj_lo, cj_hi, smask, pad;
};
typedef __attribute__((address_space(3))) const StreamLds* lds_ptr;

// a draw state as the product kernel holds it: limbs 0-1 as one VGPR pair
// (written in place by the paired draws, sa_draw3.h), limbs 2 and 3
struct MbState {
  uint64_t p01;
  uint32_t s2, s3;
};

// Same asm as pcg_draw_pair/one, but the stream constants are SGPR operands
// (scalar-loaded) and the multiplier limbs VGPR operands (gfx9 constant bus: one
// SGPR source per VOP3).
constexpr uint32_t A0 = 0x9FCCF645u, A1 = 0x4385DF64u, A2 = 0x1FC65DA4u, A3 = 0x2360ED05u;
#define SMEM_INS                                                                                         \
  [a0] "v"(a0), [a1] "v"(a1), [a2] "v"(a2), [a3] "v"(a3), [c0] "s"(inc.w0), [c1] "s"(inc.w1),             \
      [c23] "s"(inc.hi), [m] "s"(m), [mm] "s"((uint64_t)m << 32 | m)
__device__ __forceinline__ void draw_pair_s(uint32_t& s0, uint32_t& s1, uint32_t& s2, uint32_t& s3, uint32_t a0,
                                            uint32_t a1, uint32_t a2, uint32_t a3, const Inc& inc,
                                            uint32_t m, uint64_t& zs, uint64_t& u, uint64_t& v) {
  uint64_t k1, k2, k3;
  uint32_t vlo = (uint32_t)v, vhi = (uint32_t)(v >> 32);
  asm volatile(SA_PCG_DRAW_ASM
               "v_sub_co_u32_e64 %[vlo], %[k2], %[vlo], v6\n\t"
               "v_lshl_add_u64 %[u], v[6:7], 0, %[u]\n\t"
               "s_nop 0\n\t"
               "v_subb_co_u32_e64 %[vhi], %[k2], %[vhi], v7, %[k2]"
               : SA_PCG_DRAW_OUTS, [vlo] "+v"(vlo), [vhi] "+v"(vhi)
               : SMEM_INS
               : SA_PCG_DRAW_CLOBBERS);
  v = ((uint64_t)vhi << 32) | vlo;
}
__device__ __forceinline__ void draw_one_s(uint32_t& s0, uint32_t& s1, uint32_t& s2, uint32_t& s3, uint32_t a0,
                                           uint32_t a1, uint32_t a2, uint32_t a3, const Inc& inc,
                                           uint32_t m, uint64_t& zs, uint64_t& u) {
  uint64_t k1, k2, k3;
  asm volatile(SA_PCG_DRAW_ASM
               "v_lshl_add_u64 %[u], v[6:7], 0, %[u]"
               : SA_PCG_DRAW_OUTS
               : SMEM_INS
               : SA_PCG_DRAW_CLOBBERS);
}

typedef __attribute__((address_space(4))) const uint64_t* cptr_t;

// MODE 2: stream-outer tile (4 draws per stream per tile, 4 x L accumulators),
// constants scalar-loaded once per stream per tile.  PREF: load stream q+1's
// constants after stream q's first draw.
template <int P, int L, bool PAIRS, bool PREF, int E = 4>
__global__ void __launch_bounds__(256) k_smem(uint64_t* out, int iters, uint32_t seed, const uint64_t* gconst) {
  extern __shared__ char dyn[];
  if (dyn[0] == 123 && seed == 77) out[0] = 1;
  uint32_t st[P][4];
  const uint32_t tid = threadIdx.x + blockIdx.x * blockDim.x;
#pragma unroll
  for (int j = 0; j < P; j++) {
    st[j][0] = tid * 0x9E3779B9u + j;
    st[j][1] = seed ^ (j * 77u);
    st[j][2] = tid + 13u * j;
    st[j][3] = ~tid;
  }
  const uint32_t a0 = __builtin_amdgcn_readfirstlane(A0 + seed), a1 = A1, a2 = A2, a3 = A3;
  uint32_t va0, va1, va2, va3;
  asm volatile("v_mov_b32 %0, %4\n\tv_mov_b32 %1, %5\n\tv_mov_b32 %2, %6\n\tv_mov_b32 %3, %7"
               : "=v"(va0), "=v"(va1), "=v"(va2), "=v"(va3) : "s"(a0), "s"(a1), "s"(a2), "s"(a3));
  uint64_t acc2[E][L];
#pragma unroll
  for (int k = 0; k < E; k++)
#pragma unroll
    for (int c = 0; c < L; c++) acc2[k][c] = c + k;
  uint32_t zmin = 0xFFFFFFFFu;
  uint64_t zs = 0;  // single draws: lane mask of raw == 0 draws
  cptr_t cp = (cptr_t)gconst;
  for (int it = 0; it < iters; it++) {
    cptr_t f = cp;
    asm volatile("" : "+s"(f));
    Inc ninc{f[0], f[2], f[1]};
    uint64_t nm = f[4];
#pragma unroll
    for (int q = 0; q < P; q++) {
      Inc cinc = ninc;
      uint32_t sm = (uint32_t)nm;
      if constexpr (!PREF) {
        cptr_t g = cp + 8 * q;
        asm volatile("" : "+s"(g));
        cinc = Inc{g[0], g[2], g[1]};
        sm = (uint32_t)g[4];
      }
#pragma unroll
      for (int k = 0; k < E; k++) {
        if constexpr (PAIRS) {
          constexpr int PI = Pairs<L>::count;
          const int cu = Pairs<L>::u(q % PI), cv = Pairs<L>::v(q % PI);
          draw_pair_s(st[q][0], st[q][1], st[q][2], st[q][3], va0, va1, va2, va3, cinc, sm, zs, acc2[k][cu],
                      acc2[k][cv]);
        } else {
          const int cu = q % L;
          draw_one_s(st[q][0], st[q][1], st[q][2], st[q][3], va0, va1, va2, va3, cinc, sm, zs, acc2[k][cu]);
        }
        if (PREF && k == 0 && q + 1 < P) {
          cptr_t g = cp + 8 * (q + 1);
          asm volatile("" : "+s"(g));
          ninc = Inc{g[0], g[2], g[1]};
          nm = g[4];
        }
      }
    }
  }
  uint64_t acc = zmin ^ zs;
#pragma unroll
  for (int k = 0; k < E; k++)
#pragma unroll
    for (int c = 0; c < L; c++) acc += acc2[k][c];
#pragma unroll
  for (int j = 0; j < P; j++) acc ^= st[j][0] ^ st[j][3];
  out[tid] = acc;
}

// dual-draw variant of k_smem (E = 2): the kernel's Sched grouping
template <int L, int X>
__global__ void __launch_bounds__(256) k_dual(uint64_t* out, int iters, uint32_t seed, const uint64_t* gconst) {
  constexpr Sched<L, X> S{};
  constexpr int P = Sched<L, X>::P;
  extern __shared__ char dyn[];
  if (dyn[0] == 123 && seed == 77) out[0] = 1;
  MbState st[P];
  const uint32_t tid = threadIdx.x + blockIdx.x * blockDim.x;
#pragma unroll
  for (int j = 0; j < P; j++) {
    st[j].p01 = ((uint64_t)(seed ^ (j * 77u)) << 32) | (tid * 0x9E3779B9u + j);
    st[j].s2 = tid + 13u * j;
    st[j].s3 = ~tid;
  }
  const uint32_t mk[4] = {vreg(A0 + seed), vreg(A1), vreg(A2), vreg(A3)};
  uint64_t acc2[2][L];
#pragma unroll
  for (int k = 0; k < 2; k++)
#pragma unroll
    for (int c = 0; c < L; c++) acc2[k][c] = c + k;
  uint32_t zmin = 0xFFFFFFFFu;
  uint64_t zs = 0;  // single draws: lane mask of raw == 0 draws
  cptr_t cp = (cptr_t)gconst;
  for (int it = 0; it < iters; it++) {
    ZeroAcc zh = zero_acc_init();  // the paired draws' zero test, per tile as in the kernel
    Inc ninc[2];
    uint64_t nm[2];
    auto fetch = [&](int g) {
      for (int h = 0; h < 2; h++) {
        const int q = h == 0 ? S.g[g].qa : S.g[g].qb;
        if (q < 0) continue;
        cptr_t c = cp + 8 * q;
        asm volatile("" : "+s"(c));
        ninc[h] = Inc{c[0], c[2], c[1]};
        nm[h] = c[4];
      }
    };
    fetch(0);
#pragma unroll
    for (int g = 0; g < S.n; g++) {
      const Group G = S.g[g];
      const Inc ia = ninc[0], ib = ninc[1];
      const uint64_t ma = nm[0], mb = nm[1];  // 64-bit sign masks, as the kernel passes them
#pragma unroll
      for (int k = 0; k < 2; k++) {
        MbState& sa = st[G.qa];
        uint64_t* ak = acc2[k];
        const uint64_t fma_ = G.fa ? ~ma : ma, fmb_ = G.fb ? ~mb : mb;
        if (G.qb < 0) {
          uint32_t s0 = (uint32_t)sa.p01, s1 = (uint32_t)(sa.p01 >> 32);
          if (G.va >= 0 && G.va_add)
            pcg_draw_pair_a(s0, s1, sa.s2, sa.s3, mk[0], mk[1], mk[2], mk[3], ia, fma_, zs, ak[G.ua], ak[G.va]);
          else if (G.va >= 0)
            pcg_draw_pair(s0, s1, sa.s2, sa.s3, mk[0], mk[1], mk[2], mk[3], ia, fma_, zs, ak[G.ua], ak[G.va]);
          else
            pcg_draw_one(s0, s1, sa.s2, sa.s3, mk[0], mk[1], mk[2], mk[3], ia, fma_, zs, ak[G.ua]);
          sa.p01 = ((uint64_t)s1 << 32) | s0;
        } else {
          MbState& sb = st[G.qb];
#define DRAW2(fn)                                                                                         \
  fn<0>(sa.p01, sa.s2, sa.s3, sb.p01, sb.s2, sb.s3, mk[0], mk[1], mk[2], mk[3], ia, fma_, ib, fmb_, zh,       \
        ak[G.ua], ak[G.va], ak[G.ub], ak[G.vb], 0, 0, 0, 0)
          if (G.va >= 0 && G.va_add && G.vb_add)
            DRAW2(pcg_draw2_pair_aa);
          else if (G.va >= 0 && G.va_add)
            DRAW2(pcg_draw2_pair_as);
          else if (G.va >= 0 && G.vb_add)
            DRAW2(pcg_draw2_pair_sa);
          else if (G.va >= 0)
            DRAW2(pcg_draw2_pair_ss);
#undef DRAW2
          else if (G.ua == G.ub)
            pcg_draw2_one_same<0>(sa.p01, sa.s2, sa.s3, sb.p01, sb.s2, sb.s3, mk[0], mk[1], mk[2], mk[3], ia, fma_, ib,
                                  fmb_, zh, ak[G.ua], 0);
          else
            pcg_draw2_one<0>(sa.p01, sa.s2, sa.s3, sb.p01, sb.s2, sb.s3, mk[0], mk[1], mk[2], mk[3], ia, fma_, ib, fmb_,
                             zh, ak[G.ua], ak[G.ub], 0, 0);
        }
        if (k == 0 && g + 1 < S.n) fetch(g + 1);
      }
    }
    if (zero_acc_hit(zh)) zmin = 0;
  }
  uint64_t acc = zmin ^ zs;
#pragma unroll
  for (int k = 0; k < 2; k++)
#pragma unroll
    for (int c = 0; c < L; c++) acc += acc2[k][c];
#pragma unroll
  for (int j = 0; j < P; j++) acc ^= st[j].p01 ^ st[j].s3;
  out[tid] = acc;
}

// k_dual with E elements per lane and a min-waves/SIMD launch bound W: does
// a third wave per SIMD pay for the 8-client pair schedule at E = 1?
template <int L, int X, int E, int W>
__global__ void __launch_bounds__(256, W) k_dualE(uint64_t* out, int iters, uint32_t seed, const uint64_t* gconst) {
  constexpr Sched<L, X> S{};
  constexpr int P = Sched<L, X>::P;
  extern __shared__ char dyn[];
  if (dyn[0] == 123 && seed == 77) out[0] = 1;
  MbState st[P];
  const uint32_t tid = threadIdx.x + blockIdx.x * blockDim.x;
#pragma unroll
  for (int j = 0; j < P; j++) {
    st[j].p01 = ((uint64_t)(seed ^ (j * 77u)) << 32) | (tid * 0x9E3779B9u + j);
    st[j].s2 = tid + 13u * j;
    st[j].s3 = ~tid;
  }
  const uint32_t mk[4] = {vreg(A0 + seed), vreg(A1), vreg(A2), vreg(A3)};  // E = 1: the tile-jump limbs only
  uint64_t acc2[E][L];
#pragma unroll
  for (int k = 0; k < E; k++)
#pragma unroll
    for (int c = 0; c < L; c++) acc2[k][c] = c + k;
  uint32_t zmin = 0xFFFFFFFFu;
  uint64_t zs = 0;  // single draws: lane mask of raw == 0 draws
  cptr_t cp = (cptr_t)gconst;
  for (int it = 0; it < iters; it++) {
    ZeroAcc zh = zero_acc_init();  // the paired draws' zero test, per tile as in the kernel
    Inc ninc[2];
    uint64_t nm[2];
    auto fetch = [&](int g) {
      for (int h = 0; h < 2; h++) {
        const int q = h == 0 ? S.g[g].qa : S.g[g].qb;
        if (q < 0) continue;
        cptr_t c = cp + 8 * q;
        asm volatile("" : "+s"(c));
        ninc[h] = Inc{c[0], c[2], c[1]};
        nm[h] = c[4];
      }
    };
    fetch(0);
#pragma unroll
    for (int g = 0; g < S.n; g++) {
      const Group G = S.g[g];
      const Inc ia = ninc[0], ib = ninc[1];
      const uint64_t ma = nm[0], mb = nm[1];  // 64-bit sign masks, as the kernel passes them
#pragma unroll
      for (int k = 0; k < E; k++) {
        MbState& sa = st[G.qa];
        uint64_t* ak = acc2[k];
        const uint64_t fma_ = G.fa ? ~ma : ma, fmb_ = G.fb ? ~mb : mb;
        if (G.qb < 0) {
          uint32_t s0 = (uint32_t)sa.p01, s1 = (uint32_t)(sa.p01 >> 32);
          if (G.va >= 0 && G.va_add)
            pcg_draw_pair_a(s0, s1, sa.s2, sa.s3, mk[0], mk[1], mk[2], mk[3], ia, fma_, zs, ak[G.ua], ak[G.va]);
          else if (G.va >= 0)
            pcg_draw_pair(s0, s1, sa.s2, sa.s3, mk[0], mk[1], mk[2], mk[3], ia, fma_, zs, ak[G.ua], ak[G.va]);
          else
            pcg_draw_one(s0, s1, sa.s2, sa.s3, mk[0], mk[1], mk[2], mk[3], ia, fma_, zs, ak[G.ua]);
          sa.p01 = ((uint64_t)s1 << 32) | s0;
        } else {
          MbState& sb = st[G.qb];
#define DRAW2(fn)                                                                                         \
  fn<0>(sa.p01, sa.s2, sa.s3, sb.p01, sb.s2, sb.s3, mk[0], mk[1], mk[2], mk[3], ia, fma_, ib, fmb_, zh,       \
        ak[G.ua], ak[G.va], ak[G.ub], ak[G.vb], 0, 0, 0, 0)
          if (G.va >= 0 && G.va_add && G.vb_add)
            DRAW2(pcg_draw2_pair_aa);
          else if (G.va >= 0 && G.va_add)
            DRAW2(pcg_draw2_pair_as);
          else if (G.va >= 0 && G.vb_add)
            DRAW2(pcg_draw2_pair_sa);
          else if (G.va >= 0)
            DRAW2(pcg_draw2_pair_ss);
#undef DRAW2
          else if (G.ua == G.ub)
            pcg_draw2_one_same<0>(sa.p01, sa.s2, sa.s3, sb.p01, sb.s2, sb.s3, mk[0], mk[1], mk[2], mk[3], ia, fma_, ib,
                                  fmb_, zh, ak[G.ua], 0);
          else
            pcg_draw2_one<0>(sa.p01, sa.s2, sa.s3, sb.p01, sb.s2, sb.s3, mk[0], mk[1], mk[2], mk[3], ia, fma_, ib, fmb_,
                             zh, ak[G.ua], ak[G.ub], 0, 0);
        }
        if (k == 0 && g + 1 < S.n) fetch(g + 1);
      }
    }
    if (zero_acc_hit(zh)) zmin = 0;
  }
  uint64_t acc = zmin ^ zs;
#pragma unroll
  for (int k = 0; k < E; k++)
#pragma unroll
    for (int c = 0; c < L; c++) acc += acc2[k][c];
#pragma unroll
  for (int j = 0; j < P; j++) acc ^= st[j].p01 ^ st[j].s3;
  out[tid] = acc;
}

// Throughput of the draw's instruction MIX with no dependencies between
// instructions of one iteration: 6 v_mad_u64_u32 + 4 v_mul_lo_u32 + 22 simple
// ops (adds / bitop3 / alignbit / cndmask-like) per "draw" -- the issue
// ceiling the real dependency chains are measured against.
__global__ void __launch_bounds__(256) k_mix(uint64_t* out, int iters, uint32_t seed) {
  extern __shared__ char dyn[];
  if (dyn[0] == 123 && seed == 77) out[0] = 1;
  const uint32_t t = threadIdx.x + blockIdx.x * blockDim.x;
  uint64_t m[6];
  uint32_t l[4], r[22];
  uint32_t b = t * 3 + seed, c = t ^ 0x55;
  for (int j = 0; j < 6; j++) m[j] = t + j;
  for (int j = 0; j < 4; j++) l[j] = t * 7 + j;
  for (int j = 0; j < 22; j++) r[j] = t + 11 * j;
  for (int it = 0; it < iters; it++) {
    asm volatile(
        "v_mad_u64_u32 %0, s[40:41], %10, %11, %0\n\t"
        "v_add_u32 %12, %12, %11\n\t"
        "v_mad_u64_u32 %1, s[42:43], %10, %11, %1\n\t"
        "v_bitop3_b32 %13, %13, %10, %11 bitop3:0x96\n\t"
        "v_mad_u64_u32 %2, s[44:45], %10, %11, %2\n\t"
        "v_add_u32 %14, %14, %11\n\t"
        "v_mul_lo_u32 %6, %6, %11\n\t"
        "v_alignbit_b32 %15, %15, %10, %11\n\t"
        "v_mad_u64_u32 %3, s[46:47], %10, %11, %3\n\t"
        "v_add_u32 %16, %16, %11\n\t"
        "v_mul_lo_u32 %7, %7, %11\n\t"
        "v_bitop3_b32 %17, %17, %10, %11 bitop3:0x96\n\t"
        "v_mad_u64_u32 %4, s[48:49], %10, %11, %4\n\t"
        "v_add_u32 %18, %18, %11\n\t"
        "v_mul_lo_u32 %8, %8, %11\n\t"
        "v_alignbit_b32 %19, %19, %10, %11\n\t"
        "v_mad_u64_u32 %5, s[50:51], %10, %11, %5\n\t"
        "v_add_u32 %20, %20, %11\n\t"
        "v_mul_lo_u32 %9, %9, %11\n\t"
        "v_bitop3_b32 %21, %21, %10, %11 bitop3:0x96\n\t"
        "v_add_u32 %22, %22, %11\n\t"
        "v_add_u32 %23, %23, %11\n\t"
        "v_bitop3_b32 %24, %24, %10, %11 bitop3:0x96\n\t"
        "v_add_u32 %25, %25, %11\n\t"
        "v_alignbit_b32 %26, %26, %10, %11\n\t"
        "v_add_u32 %27, %27, %11\n\t"
        "v_add_u32 %28, %28, %11\n\t"
        "v_bitop3_b32 %29, %29, %10, %11 bitop3:0x96\n\t"
        "v_add_u32 %30, %30, %11\n\t"
        "v_add_u32 %31, %31, %11\n\t"
        "v_add_u32 %32, %32, %11\n\t"
        "v_add_u32 %33, %33, %11"
        : "+v"(m[0]), "+v"(m[1]), "+v"(m[2]), "+v"(m[3]), "+v"(m[4]), "+v"(m[5]), "+v"(l[0]), "+v"(l[1]),
          "+v"(l[2]), "+v"(l[3]), "+v"(b), "+v"(c), "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]),
          "+v"(r[5]), "+v"(r[6]), "+v"(r[7]), "+v"(r[8]), "+v"(r[9]), "+v"(r[10]), "+v"(r[11]), "+v"(r[12]),
          "+v"(r[13]), "+v"(r[14]), "+v"(r[15]), "+v"(r[16]), "+v"(r[17]), "+v"(r[18]), "+v"(r[19]),
          "+v"(r[20]), "+v"(r[21])
        :
        : "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50", "s51");
  }
  uint64_t acc = 0;
  for (int j = 0; j < 6; j++) acc += m[j];
  for (int j = 0; j < 4; j++) acc += l[j];
  for (int j = 0; j < 22; j++) acc ^= r[j];
  out[t] = acc;
}

// MODE 0: constants in VGPRs (loaded once);  MODE 1: constants from LDS per draw
// (the product kernel's scheme).  PAIRS: internal pair draws into L accumulators.
template <int P, int L, bool PAIRS, int MODE>
__global__ void __launch_bounds__(256) k_draws(uint64_t* out, int iters, uint32_t seed) {
  extern __shared__ char dyn[];  // occupancy limiter only
  __shared__ StreamLds sl[P];
  for (int j = threadIdx.x; j < P; j += blockDim.x)
    sl[j] = StreamLds{2ull * j + 1 + seed, (uint64_t)j << 7, 3ull * j, 0, (j & 1) ? ~0ull : 0ull, 0};
  __syncthreads();
  if (dyn[0] == 123 && seed == 77) out[0] = 1;  // keep the dynamic LDS allocation

  uint32_t st[P][4];
  const uint32_t tid = threadIdx.x + blockIdx.x * blockDim.x;
#pragma unroll
  for (int j = 0; j < P; j++) {
    st[j][0] = tid * 0x9E3779B9u + j;
    st[j][1] = seed ^ (j * 77u);
    st[j][2] = tid + 13u * j;
    st[j][3] = ~tid;
  }
  Inc rinc[MODE == 0 ? P : 1];
  uint64_t rm[MODE == 0 ? P : 1];
  if constexpr (MODE == 0) {
#pragma unroll
    for (int j = 0; j < P; j++) {
      rinc[j] = Inc{(uint32_t)sl[j].inc_lo, sl[j].inc_lo >> 32, sl[j].inc_hi};
      rm[j] = sl[j].smask;
    }
  }
  uint64_t acc1[L];
#pragma unroll
  for (int c = 0; c < L; c++) acc1[c] = c;
  uint32_t zmin = 0xFFFFFFFFu;
  uint64_t zs = 0;  // single draws: lane mask of raw == 0 draws
  lds_ptr slp = (lds_ptr)(sl);
  for (int it = 0; it < iters; it++) {
#pragma unroll
    for (int q = 0; q < P; q++) {
      Inc cinc;
      uint64_t sm;
      if constexpr (MODE == 0) {
        cinc = rinc[q];
        sm = rm[q];
      } else {
        asm volatile("" : "+v"(slp));
        typedef __attribute__((address_space(3))) const uint64_t* lds_u64;
        const lds_u64 cp = (lds_u64)(slp + q);
        cinc = Inc{(uint32_t)cp[0], cp[0] >> 32, cp[1]};
        sm = slp[q].smask;
      }
      if constexpr (PAIRS) {
        constexpr int PI = Pairs<L>::count;
        const int cu = Pairs<L>::u(q % PI), cv = Pairs<L>::v(q % PI);
        pcg_draw_pair(st[q][0], st[q][1], st[q][2], st[q][3], A0, A1, A2, A3, cinc, sm, zs, acc1[cu],
                      acc1[cv]);
      } else {
        const int cu = q % L;
        pcg_draw_one(st[q][0], st[q][1], st[q][2], st[q][3], A0, A1, A2, A3, cinc, sm, zs, acc1[cu]);
      }
    }
  }
  uint64_t acc = zmin ^ zs;
#pragma unroll
  for (int c = 0; c < L; c++) acc += acc1[c];
#pragma unroll
  for (int j = 0; j < P; j++) acc ^= st[j][0] ^ st[j][3];
  out[tid] = acc;
}

// usage: draw_issue                     all cases, every occupancy
//        draw_issue CASE WAVES         one case at one occupancy: the median
//                                      of 15 launches after 40 warm-up ones, as
//                                      one JSON line (bench.py measures the
//                                      same-box draw-loop ceiling)
int main(int argc, char** argv) {
  const char* only = argc > 1 ? argv[1] : nullptr;
  const int only_w = argc > 2 ? atoi(argv[2]) : 0;
  int ncu = 0;
  CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0));
  uint64_t* d_out;
  CHECK(hipMalloc(&d_out, (size_t)ncu * 8 * 256 * sizeof(uint64_t)));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  uint64_t* gconst;
  CHECK(hipMalloc(&gconst, 64 * 64));
  {
    uint64_t h[64 * 8];
    for (int j = 0; j < 64; j++) {
      h[8 * j + 0] = 2ull * j + 7;
      h[8 * j + 1] = (uint64_t)j << 7;
      h[8 * j + 2] = 3ull * j;  // the increment's second word (zero-extended)
      h[8 * j + 3] = 0;
      h[8 * j + 4] = (j & 1) ? ~0ull : 0ull;
      h[8 * j + 5] = h[8 * j + 6] = h[8 * j + 7] = 0;
    }
    CHECK(hipMemcpy(gconst, h, sizeof(h), hipMemcpyHostToDevice));
  }
  auto run = [&](auto kern, int P, const char* name, int iters, auto... extra) -> int {
    if (only && strcmp(only, name) != 0) return 0;
    for (int w : {1, 2, 3, 4, 5, 6, 8}) {
      if (only_w && w != only_w) continue;
      // w blocks of 4 waves per CU -> w waves per SIMD (if registers allow)
      const size_t dyn = (160 * 1024) / w - 4096;
      int nb = 0;
      CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, 256, dyn));
      if (nb < w) {
        printf("%-22s waves/SIMD=%d  not reachable (max %d)\n", name, w, nb);
        continue;
      }
      const int blocks = ncu * w;
      float ms = 0;
      // one case: 40 untimed launches first (clocks ramp up from idle over
      // the first ~10 ms), then the median of 15
      const int reps = only ? 15 : 2;
      float t[15];
      for (int rep = 0; only && rep < 40; rep++)
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), dyn, 0, d_out, iters, 5u, extra...);
      for (int rep = 0; rep < reps; rep++) {
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), dyn, 0, d_out, iters, 5u, extra...);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&t[rep], e0, e1));
      }
      if (only) std::sort(t, t + reps);
      ms = only ? t[reps / 2] : t[reps - 1];  // one case: the median; the sweep: the second launch
      const double draws = (double)blocks * 256 * iters * P;
      if (only) {
        printf("{\"case\": \"%s\", \"waves_per_simd\": %d, \"ms\": %.4f, \"draws_per_s\": %.6e}\n", name, w, ms,
               draws / (ms * 1e-3));
        continue;
      }
      printf("%-22s waves/SIMD=%d  %8.3f ms  %7.1f G draws/s\n", name, w, ms, draws / (ms * 1e-3) / 1e9);
      fflush(stdout);
    }
    return 0;
  };
  if (run(k_draws<7, 1, false, 0>, 7, "one7 L1 reg", 4000)) return 1;
  if (run(k_draws<7, 1, false, 1>, 7, "one7 L1 lds", 4000)) return 1;
  if (run(k_draws<28, 8, true, 1>, 28, "pair28 L8 lds", 1000)) return 1;
  if (run(k_draws<28, 8, true, 0>, 28, "pair28 L8 reg", 1000)) return 1;
  const uint64_t* gc = gconst;
  if (run(k_mix, 1, "mix 10mul+22simple", 20000)) return 1;
  if (run(k_dual<1, 7>, 14, "dual one7 E2", 1000, gc)) return 1;
  if (run(k_dual<8, 0>, 56, "dual pair28 E2", 250, gc)) return 1;
  if (run(k_dual<4, 4>, 44, "dual 4+4x4 E2", 300, gc)) return 1;
  if (run(k_dualE<8, 0, 1, 2>, 28, "dual pair28 E1 W2", 500, gc)) return 1;
  if (run(k_dualE<8, 0, 1, 3>, 28, "dual pair28 E1 W3", 500, gc)) return 1;
  if (run(k_dualE<8, 0, 2, 3>, 56, "dual pair28 E2 W3", 250, gc)) return 1;
  if (run(k_smem<7, 1, false, true, 4>, 28, "one7 L1 smem E4", 1000, gc)) return 1;
  if (run(k_smem<7, 1, false, true, 1>, 7, "one7 L1 smem E1", 4000, gc)) return 1;
  if (run(k_smem<7, 1, false, true, 2>, 14, "one7 L1 smem E2", 2000, gc)) return 1;
  if (run(k_smem<28, 8, true, true, 4>, 112, "pair28 L8 smem E4", 250, gc)) return 1;
  if (run(k_smem<28, 8, true, true, 2>, 56, "pair28 L8 smem E2", 500, gc)) return 1;
  if (run(k_smem<28, 8, true, true, 1>, 28, "pair28 L8 smem E1", 1000, gc)) return 1;
  CHECK(hipGetLastError());
  return 0;
}
