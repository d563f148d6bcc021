// pcg128.h — 128-bit LCG algebra for numpy's PCG64 (XSL-RR 128/64), usable on
// host and device and in constant expressions.
//
// numpy's PCG64 (numpy/random/src/pcg64/pcg64.h, the generator the reference
// names in docs/developer/algorithm/secure_aggregation.ipynb cell 15) steps
//     s <- s * A + inc   (mod 2^128),  A = 0x2360ED051FC65DA4_4385DF649FCCF645
// and emits rotr64(hi(s) ^ lo(s), hi(s) >> 58) of the NEW state.  Because the
// step is affine, k steps are s <- A^k s + inc * G_k with G_k = sum_{j<k} A^j,
// so any element of a mask stream is reachable in O(log k) (jump-ahead) and a
// GPU lane can start its stream at its own element with no inter-lane state.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SA_HD __host__ __device__
#else
#define SA_HD
#endif

namespace sa {

typedef unsigned __int128 u128;

constexpr u128 mk128(uint64_t hi, uint64_t lo) { return ((u128)hi << 64) | lo; }
constexpr uint64_t lo64(u128 x) { return (uint64_t)x; }
constexpr uint64_t hi64(u128 x) { return (uint64_t)(x >> 64); }

constexpr u128 kPcgMult = mk128(0x2360ED051FC65DA4ULL, 0x4385DF649FCCF645ULL);
// Generator.integers(int64.min, int64.max) == raw + kMaskOffset (mod 2^64)
// (numpy Lemire bounded draw with rng = 2^64-2; raw == 0 is rejected).
constexpr uint64_t kMaskOffset = 0x7FFFFFFFFFFFFFFFULL;

// An affine jump: s -> mult * s + plus_unit * inc.  `plus_unit` (= G_k) is
// independent of the stream's increment, so one table serves every stream.
struct Jump {
  u128 mult;  // A^k
  u128 gsum;  // G_k = sum_{j<k} A^j
};

// compose: first apply `a`, then `b`   (b ∘ a)
SA_HD constexpr Jump compose(Jump a, Jump b) {
  return Jump{b.mult * a.mult, b.mult * a.gsum + b.gsum};
}

SA_HD constexpr Jump jump_of(uint64_t k_lo, uint64_t k_hi = 0) {
  Jump acc{1, 0};
  Jump cur{kPcgMult, 1};
  u128 k = mk128(k_hi, k_lo);
  while (k) {
    if (k & 1) acc = compose(acc, cur);
    cur = compose(cur, cur);
    k >>= 1;
  }
  return acc;
}

SA_HD constexpr u128 apply(Jump j, u128 s, u128 inc) { return j.mult * s + j.gsum * inc; }

SA_HD constexpr uint64_t rotr64(uint64_t x, unsigned r) {
  return (x >> (r & 63)) | (x << ((64 - r) & 63));
}
SA_HD constexpr uint64_t xslrr(u128 s) { return rotr64(hi64(s) ^ lo64(s), (unsigned)(hi64(s) >> 58)); }

// inverse of an odd value mod 2^128 (Newton: x <- x(2 - a x) doubles the
// correct low bits; a*a == 1 mod 8 for odd a, so 6 steps reach 192 > 128)
SA_HD constexpr u128 inv128(u128 a) {
  u128 x = a;
  for (int i = 0; i < 6; i++) x *= (u128)2 - a * x;
  return x;
}

constexpr int kBlockThreads = 256;  // masking-kernel workgroup
constexpr int kDpBlock = 4;         // elements per Philox counter block (DP noise)
constexpr int kE = 2;                      // masking kernel: elements per lane per tile
constexpr int kTile = kBlockThreads * kE;  // elements per workgroup tile (512)

// The masking kernel's draw (sa_draw3.h, SA_PCG_DRAW_ASM) forms the weight-2^32
// column of S * M + C as O1 = s0*a1 + c1 + s1*a0 in ONE 64-bit register pair
// and drops the carry out of it.  With 32-bit limbs and c1 < 2^32,
// O1 <= (2^32 - 1)(a0 + a1 + 1), below 2^64 exactly when a0 + a1 + 1 <= 2^32
// (a0, a1: the multiplier's two low limbs; tight -- at 2^32 + 2 the all-ones
// state overflows).  The draw is correct only for such a multiplier.
SA_HD constexpr bool carry_free(u128 mult) {
  return (uint64_t)(uint32_t)mult + (uint64_t)(uint32_t)(mult >> 32) + 1 <= ((uint64_t)1 << 32);
}
static_assert(carry_free(kPcgMult), "PCG64's multiplier: the plain step's three-carry draw");

// The masking launch's grid.  A tile's first element is reached by the merged
// tile jump A^J, J = grid * kTile - (kE - 1) draws, so the grid decides whether
// that multiplier is carry-free.  Among 1..cap: the smallest grid >=
// min(tiles, cap) whose jump qualifies (a block without a tile runs no
// iteration, so a few idle blocks are free); if there is none up to cap, the
// largest qualifying grid below; 0 if none at all.  (Of the grids 1..2048,
// 1,048 qualify and no run of non-qualifying ones is longer than 8.)
SA_HD constexpr bool grid_carry_free(uint64_t grid) {
  return carry_free(jump_of(grid * kTile - (kE - 1)).mult);
}
SA_HD constexpr int qualifying_grid(uint64_t tiles, int cap) {
  if (cap < 1) return 0;
  const int want = tiles < (uint64_t)cap ? (tiles < 1 ? 1 : (int)tiles) : cap;
  for (int g = want; g <= cap; g++)
    if (grid_carry_free((uint64_t)g)) return g;
  for (int g = want - 1; g >= 1; g--)
    if (grid_carry_free((uint64_t)g)) return g;
  return 0;
}
static_assert(qualifying_grid(1, 512) == 2 && qualifying_grid(6, 512) == 8 && qualifying_grid(7, 512) == 8 &&
                  qualifying_grid(9, 512) == 11 && qualifying_grid(16, 512) == 20 &&
                  qualifying_grid(64, 512) == 64 && qualifying_grid(512, 512) == 512 &&
                  qualifying_grid(1000000, 512) == 512 && qualifying_grid(1000000, 511) == 508 &&
                  qualifying_grid(1000000, 496) == 495 && qualifying_grid(1000000, 256) == 255,
              "grid choices, checked against pow(A, g * 512 - 1, 2^128)");

}  // namespace sa
