// sa_ppb.h — multi-precision integers for PPBAggregator's Paillier kernels
// (sa_ppb.hip; the contract is in include/sfl_sa.h, the design in DESIGN.md
// §24).
//
// A number of L 32-bit limbs is held by a GROUP of G = L / W neighbouring
// lanes of one wave, lane g of the group holding limbs g W .. g W + W - 1 in
// registers (W = 8 for L >= 32, else 4: 16 lanes a number at L = 128, one lane
// at L = 4; a wave always carries 64 / G numbers).  Everything below is
// called by all lanes of a wave together; the only traffic between lanes is
// __shfl inside a group.
//
// montmul(a, b) = a b R^-1 mod m, R = 2^(32 L), m odd, a, b < m, limb-serial
// over b (one limb broadcast from its owner a step).  A step is
//   t[k]  = a[k] b_i + acc[k]             one v_mad_u64_u32 a limb; acc[k] is a
//                                         column sum below 2^33, so t fits 64 bits
//   s[k]  = lo(t[k]) + hi(t[k - 1])       hi(t[-1]) from the lane below
//   q     = lo(s[0]) m' of the group's lane 0, broadcast (m' = -m^-1 mod 2^32)
//   u[k]  = m[k] q + s[k]                 one v_mad_u64_u32 a limb
//   acc[k] = lo(u[k + 1]) + hi(u[k])      lo(u[W]) from the lane above: the
//                                         division by 2^32 is this shift
// so no carry travels along the number inside a step: every column keeps its
// carry as the 33rd bit of its sum, and the sums are resolved once a
// multiplication (normalize), followed by the conditional subtraction of m.
// The top lane keeps one more column, X, for what leaves the top limb.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sa {
namespace ppb {

constexpr int kWave = 64;
constexpr int kWindow = 4;  // exponent bits a table look-up (16 powers in LDS)

template <int G>
__device__ __forceinline__ uint32_t from_lane(uint32_t v, int src) {
  return G == 1 ? v : (uint32_t)__shfl((int)v, src, G);
}
// the value of the group's lane below / above; 0 at the group's end
template <int G>
__device__ __forceinline__ uint32_t from_below(uint32_t v, int gl) {
  if (G == 1) return 0;
  const uint32_t r = (uint32_t)__shfl_up((int)v, 1, G);
  return gl == 0 ? 0u : r;
}
template <int G>
__device__ __forceinline__ uint32_t from_above(uint32_t v, int gl) {
  if (G == 1) return 0;
  const uint32_t r = (uint32_t)__shfl_down((int)v, 1, G);
  return gl == G - 1 ? 0u : r;
}

__device__ __forceinline__ uint32_t lo32(uint64_t v) { return (uint32_t)v; }
__device__ __forceinline__ uint32_t hi32(uint64_t v) { return (uint32_t)(v >> 32); }

// Column sums (each far below 2^63) to limbs; returns what leaves the top
// limb, the same value in every lane of the group.  A lane ripples its own
// columns, then the lanes' carries move up one lane a round until none is
// left in the wave (at most G rounds: a carry only moves upwards).
template <int G, int W>
__device__ __forceinline__ uint32_t normalize(const uint64_t (&col)[W], uint32_t (&limb)[W], int gl) {
  uint64_t c = 0;
#pragma unroll
  for (int k = 0; k < W; k++) {
    const uint64_t v = col[k] + c;
    limb[k] = lo32(v);
    c = v >> 32;
  }
  uint32_t out = (uint32_t)c, top = 0;
  for (int round = 0; round <= G; round++) {
    if (gl == G - 1) top += out;
    const uint32_t in = from_below<G>(out, gl);
    if (!__any(in != 0)) break;
    uint64_t cc = in;
#pragma unroll
    for (int k = 0; k < W; k++) {
      const uint64_t v = (uint64_t)limb[k] + cc;
      limb[k] = lo32(v);
      cc = v >> 32;
    }
    out = (uint32_t)cc;
  }
  return from_lane<G>(top, G - 1);
}

// r = r - m when r + top 2^(32 L) >= m (the caller knows the result is below m)
template <int G, int W>
__device__ __forceinline__ void reduce_once(uint32_t (&r)[W], uint32_t top, const uint32_t (&m)[W], int gl) {
  uint64_t col[W];
  uint32_t d[W];
#pragma unroll
  for (int k = 0; k < W; k++) col[k] = (uint64_t)r[k] + (uint32_t)~m[k];
  if (gl == 0) col[0] += 1;
  const uint32_t ge = top | normalize<G, W>(col, d, gl);
#pragma unroll
  for (int k = 0; k < W; k++) r[k] = ge ? d[k] : r[k];
}

// out = a b R^-1 mod m.  q, when given, receives the steps' quotient digits
// as a number (digit i is limb i): for b = 1 they are -a / m mod R when m
// divides a, the exact division of sa_ppb_decrypt.  out may be a or b.
template <int G, int W, bool kDigits = false>
__device__ __forceinline__ void montmul(const uint32_t (&a)[W], const uint32_t (&b)[W], const uint32_t (&m)[W],
                                        uint32_t minv, uint32_t (&out)[W], int gl, uint32_t* q = nullptr) {
  uint64_t acc[W];
#pragma unroll
  for (int k = 0; k < W; k++) acc[k] = 0;
  uint32_t x = 0;  // the top lane's column L
#pragma unroll 1
  for (int s = 0; s < G; s++) {
#pragma unroll
    for (int j = 0; j < W; j++) {
      const uint32_t bi = from_lane<G>(b[j], s);
      uint64_t t[W];
#pragma unroll
      for (int k = 0; k < W; k++) t[k] = (uint64_t)a[k] * bi + acc[k];
      uint64_t sc[W];
      sc[0] = (uint64_t)lo32(t[0]) + from_below<G>(hi32(t[W - 1]), gl);
#pragma unroll
      for (int k = 1; k < W; k++) sc[k] = (uint64_t)lo32(t[k]) + hi32(t[k - 1]);
      const uint64_t sx = (uint64_t)x + hi32(t[W - 1]);
      const uint32_t qd = from_lane<G>(lo32(sc[0]) * minv, 0);
      uint64_t u[W];
#pragma unroll
      for (int k = 0; k < W; k++) u[k] = (uint64_t)m[k] * qd + sc[k];
      uint32_t above = from_above<G>(lo32(u[0]), gl);
      if (gl == G - 1) above = lo32(sx);
#pragma unroll
      for (int k = 0; k + 1 < W; k++) acc[k] = (uint64_t)lo32(u[k + 1]) + hi32(u[k]);
      acc[W - 1] = (uint64_t)above + hi32(u[W - 1]);
      x = hi32(sx);
      if (kDigits && gl == s) q[j] = qd;
    }
  }
  uint32_t top = normalize<G, W>(acc, out, gl);
  top += from_lane<G>(x, G - 1);
  reduce_once<G, W>(out, top, m, gl);
}

// a lane's W limbs of a row of `limbs` limbs at p (zero above the row's end)
template <int W>
__device__ __forceinline__ void load_limbs(const uint32_t* p, int limbs, int gl, uint32_t (&v)[W]) {
#pragma unroll
  for (int k = 0; k < W; k++) v[k] = gl * W + k < limbs ? p[gl * W + k] : 0u;
}
template <int W>
__device__ __forceinline__ void store_limbs(uint32_t* p, int limbs, int gl, const uint32_t (&v)[W]) {
#pragma unroll
  for (int k = 0; k < W; k++)
    if (gl * W + k < limbs) p[gl * W + k] = v[k];
}

// The modulus of a launch and what goes with it, in registers.
template <int W>
struct Mod {
  uint32_t m[W], r2[W], one[W];  // m, R^2 mod m, R mod m
  uint32_t minv;
};

// out = base^e R mod m (Montgomery form), e of `ebits` bits at `exp` (little-
// endian limbs; every number of the launch shares it, so the wave's control
// flow is uniform).  Fixed windows of kWindow bits from the top; the 16
// powers base^0..15 in Montgomery form in the lane's own slots of `tab`
// (16 x 64 x W words of LDS: written and read by the same lane, no barrier).
template <int G, int W>
__device__ __forceinline__ void modexp(const uint32_t (&base)[W], const Mod<W>& md, const uint32_t* exp, int ebits,
                                       uint32_t* tab, uint32_t (&out)[W], int gl) {
  constexpr int kPowers = 1 << kWindow;
  uint32_t* mine = tab + threadIdx.x * W;
  auto slot = [&](int e) { return mine + e * kWave * W; };
  uint32_t b1[W], cur[W];
  montmul<G, W>(base, md.r2, md.m, md.minv, b1, gl);
#pragma unroll
  for (int k = 0; k < W; k++) {
    slot(0)[k] = md.one[k];
    slot(1)[k] = b1[k];
    cur[k] = b1[k];
  }
#pragma unroll 1
  for (int e = 2; e < kPowers; e++) {
    montmul<G, W>(cur, b1, md.m, md.minv, cur, gl);
#pragma unroll
    for (int k = 0; k < W; k++) slot(e)[k] = cur[k];
  }
  const int windows = (ebits + kWindow - 1) / kWindow;
  auto window = [&](int i) { return (int)((exp[(i * kWindow) >> 5] >> ((i * kWindow) & 31)) & (kPowers - 1)); };
  {
    const uint32_t* p = slot(windows > 0 ? window(windows - 1) : 0);
#pragma unroll
    for (int k = 0; k < W; k++) out[k] = p[k];
  }
#pragma unroll 1
  for (int i = windows - 2; i >= 0; i--) {
    const uint32_t* p = slot(window(i));
#pragma unroll 1
    for (int it = 0; it <= kWindow; it++) {  // kWindow squarings, then the table's power
      uint32_t b[W];
#pragma unroll
      for (int k = 0; k < W; k++) b[k] = it < kWindow ? out[k] : p[k];
      montmul<G, W>(out, b, md.m, md.minv, out, gl);
    }
  }
}

}  // namespace ppb
}  // namespace sa
