// sa_chacha.h — cryptographically secure Gaussian noise for the DP pre-step
// (GaussianModelDP's is_secure_generator; the contract is in
// include/sfl_sa.h).
//
// ChaCha20 (RFC 8439 section 2.3) with a 64-bit block counter in state words
// 12, 13 and a 64-bit nonce in words 14, 15 maps (key, nonce, block) -> 16
// uint32.  Four words make one normal (two 53-bit uniforms, Box-Muller, the
// pair combined as Holohan and Braghin describe), so a block makes four:
// element e of a vector takes normal (e & 3) of block e >> 2, the indexing
// of sa_philox.h.  The block function compiles for the host too
// (sa_chacha20_blocks_host, the known-answer tests).
#pragma once
#include <stdint.h>

namespace sa {

#if defined(__HIPCC__)
#define SA_CC_HD __host__ __device__
#else
#define SA_CC_HD
#endif

// rotate left by n: one v_alignbit_b32 on the device ({x, x} >> (32 - n))
template <int n>
SA_CC_HD inline uint32_t rotl32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(x, x, 32 - n);
#else
  return (x << n) | (x >> (32 - n));
#endif
}

SA_CC_HD inline void chacha_quarter(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
  a += b; d ^= a; d = rotl32<16>(d);
  c += d; b ^= c; b = rotl32<12>(b);
  a += b; d ^= a; d = rotl32<8>(d);
  c += d; b ^= c; b = rotl32<7>(b);
}

// o[0..15] = the ChaCha20 block `blk` under (key, nonce): 10 double rounds
// (column, diagonal), then the input state added.  On the device key and
// nonce are kernel arguments (uniform: they stay in SGPRs); only the two
// counter words differ between lanes.
SA_CC_HD inline void chacha20_block(const uint32_t key[8], uint64_t nonce, uint64_t blk, uint32_t o[16]) {
  uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u,
                     key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7],
                     (uint32_t)blk, (uint32_t)(blk >> 32), (uint32_t)nonce, (uint32_t)(nonce >> 32)};
#pragma unroll
  for (int i = 0; i < 16; i++) o[i] = in[i];
#pragma unroll
  for (int r = 0; r < 10; r++) {
    chacha_quarter(o[0], o[4], o[8], o[12]);
    chacha_quarter(o[1], o[5], o[9], o[13]);
    chacha_quarter(o[2], o[6], o[10], o[14]);
    chacha_quarter(o[3], o[7], o[11], o[15]);
    chacha_quarter(o[0], o[5], o[10], o[15]);
    chacha_quarter(o[1], o[6], o[11], o[12]);
    chacha_quarter(o[2], o[7], o[8], o[13]);
    chacha_quarter(o[3], o[4], o[9], o[14]);
  }
#pragma unroll
  for (int i = 0; i < 16; i++) o[i] += in[i];
}

#if defined(__HIPCC__)
// One normal of standard deviation sigma from four keystream words, every
// step a rounded float64 operation in the reference's order
// (distrbutions.py:124-137; the build has -ffp-contract=off): u1 feeds the
// angle, u2 the radius; 1 - u2 is in (0, 1], so the logarithm is finite;
// sigma multiplies each Box-Muller output before they are summed.  The
// square root and the division are the correctly rounded IEEE operations;
// log / sin / cos are the device math library's (theta < 2 pi: their small-
// argument paths).  sa_hb_normals_f64 and the perturb kernel both call this.
// (always_inline spelled out: sa_host.cpp includes this file without the HIP
// runtime header that defines __forceinline__.)
__device__ inline __attribute__((always_inline)) double hb_normal(uint32_t a, uint32_t b, uint32_t c, uint32_t d, double sigma) {
  const double u1 = (double)((((uint64_t)b << 32) | a) >> 11) * 0x1p-53;
  const double u2 = (double)((((uint64_t)d << 32) | c) >> 11) * 0x1p-53;
  const double r = __dsqrt_rn(-2.0 * log(1.0 - u2));
  const double theta = (2.0 * 3.141592653589793) * u1;
  const double n1 = (r * sin(theta)) * sigma;
  const double n2 = (r * cos(theta)) * sigma;
  return __ddiv_rn(n1 + n2, 1.4142135623730951);  // math.sqrt(2.0)
}
#endif

}  // namespace sa
