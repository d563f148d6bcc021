// sa_ppb.hip — PPBAggregator on the device: batched Paillier aggregation (the
// reference's phe_paillier_batch_aggregator, sfl/security/aggregation/
// experiment/ppb_aggregator.py:249-420; sfl_amd/security/aggregation/
// ppb_aggregator.py has the definition and the host form, include/sfl_sa.h the
// contract, DESIGN.md §24 the design and the compiled resources).
//
//   k_encode   one thread an output limb: the (at most two) 55-bit fields
//              that overlap it, each int(|x w / total + bias| expand) in
//              float64, and the three refusals as flag bits
//   k_encrypt  one lane group a ciphertext (sa_ppb.h): r by ChaCha20 and
//              rejection, r^n mod n^2 by the windowed exponentiation,
//              1 + m n as montmul(m, n R) + 1, and their product
//   k_add      the product of C ciphertexts: 2 (C - 1) Montgomery products
//   k_pow      c^lambda mod n^2 into scratch, then
//   k_lmu      on K / 32 limbs: (x - 1) / n exactly, as the negated quotient
//              digits of one Montgomery reduction of x - 1 mod 2^K by n, and
//              the product with mu mod n
//   k_decode   one thread an element: its field, / expand - C bias
// The exponentiating kernels run one wave a block (the table of powers takes
// 4 KiB of LDS a limb held, 32 KiB at W = 8); a wave holds 64 / G numbers.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/sfl_sa.h"
#include "sa_chacha.h"
#include "sa_internal.h"
#include "sa_ppb.h"

namespace {

using namespace sa::ppb;

constexpr int kHeader = 8;  // words in front of the key's numbers
// the key's constants (uint32 words; LN = K / 32): what the host writes
struct Consts {
  const uint32_t* p;
  int ln;
  __host__ __device__ uint32_t minv_n2() const { return p[1]; }
  __host__ __device__ uint32_t minv_n() const { return p[2]; }
  __host__ __device__ int lambda_bits() const { return (int)p[3]; }
  __host__ __device__ const uint32_t* n2() const { return p + kHeader; }
  __host__ __device__ const uint32_t* r2() const { return p + kHeader + 2 * ln; }
  __host__ __device__ const uint32_t* one() const { return p + kHeader + 4 * ln; }
  __host__ __device__ const uint32_t* nr() const { return p + kHeader + 6 * ln; }
  __host__ __device__ const uint32_t* n() const { return p + kHeader + 8 * ln; }
  __host__ __device__ const uint32_t* lambda() const { return p + kHeader + 9 * ln; }
  __host__ __device__ const uint32_t* mu_r() const { return p + kHeader + 10 * ln; }
};
constexpr int consts_words(int key_bits) { return kHeader + 11 * (key_bits / 32); }

struct Key {
  uint32_t w[8];
};
struct Tables {
  const uint32_t* ct[SA_PPB_MAX_PARTIES];
};

template <int W>
__device__ __forceinline__ Mod<W> mod_n2(const Consts& c, int gl) {
  Mod<W> md;
  load_limbs<W>(c.n2(), 2 * c.ln, gl, md.m);
  load_limbs<W>(c.r2(), 2 * c.ln, gl, md.r2);
  load_limbs<W>(c.one(), 2 * c.ln, gl, md.one);
  md.minv = c.minv_n2();
  return md;
}

// the wave's numbers: group g of the block takes row block * (64 / G) + g; a
// group past the end repeats the last row (every lane stays in the wave's
// shuffles and votes) and stores nothing
template <int G>
__device__ __forceinline__ uint64_t my_row(uint64_t rows, bool* live) {
  const uint64_t row = (uint64_t)blockIdx.x * (kWave / G) + threadIdx.x / G;
  *live = row < rows;
  return *live ? row : rows - 1;
}

// ------------------------------------------------------------------ encrypt
template <int L, int W>
__global__ __launch_bounds__(kWave) void k_encrypt(const uint32_t* plain, uint64_t rows, Consts c, Key key,
                                                   uint64_t nonce, uint32_t* out, uint32_t* flags) {
  constexpr int G = L / W, LN = L / 2;
  __shared__ uint32_t tab[(1 << kWindow) * kWave * W];
  const int gl = threadIdx.x % G;
  bool live;
  const uint64_t row = my_row<G>(rows, &live);
  const Mod<W> md = mod_n2<W>(c, gl);
  uint32_t nn[W];
  load_limbs<W>(c.n(), LN, gl, nn);

  // r: the first of 64 candidates with 0 < r < n; candidate t is the first
  // LN words of the keystream from block (64 row + t) ceil(K / 512)
  constexpr uint64_t kBlocks = (LN + 15) / 16;
  uint32_t r[W];
#pragma unroll
  for (int k = 0; k < W; k++) r[k] = 0;
  bool found = false;
#pragma unroll 1
  for (int t = 0; t < 64; t++) {
    uint32_t o[16], cand[W];
    sa::chacha20_block(key.w, nonce, (64 * row + t) * kBlocks + (uint64_t)((gl * W) / 16), o);
#pragma unroll
    for (int k = 0; k < W; k++) cand[k] = 0;
#pragma unroll
    for (int at = 0; at < 16; at += W)
      if ((gl * W) % 16 == at && gl * W < LN) {
#pragma unroll
        for (int k = 0; k < W; k++) cand[k] = o[at + k];
      }
    uint32_t any = 0;
    uint64_t col[W];
#pragma unroll
    for (int k = 0; k < W; k++) {
      any |= cand[k];
      col[k] = (uint64_t)cand[k] + (uint32_t)~nn[k];
    }
    if (gl == 0) col[0] += 1;
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) any |= (uint32_t)__shfl_xor((int)any, off, G);
    uint32_t d[W];
    const bool below = normalize<G, W>(col, d, gl) == 0;  // no carry out of cand - n: cand < n
    if (!found && any != 0 && below) {
      found = true;
#pragma unroll
      for (int k = 0; k < W; k++) r[k] = cand[k];
    }
    if (__all(found)) break;
  }
  if (!found && live && gl == 0) atomicOr(flags, SA_PPB_FLAG_NO_R);

  uint32_t rn[W], m[W], nr[W], gm[W];
  modexp<G, W>(r, md, c.n(), 32 * LN, tab, rn, gl);  // r^n R
  load_limbs<W>(plain + row * LN, LN, gl, m);
  load_limbs<W>(c.nr(), L, gl, nr);
  montmul<G, W>(m, nr, md.m, md.minv, gm, gl);  // m n (below n^2: exact)
  uint64_t col[W];
#pragma unroll
  for (int k = 0; k < W; k++) col[k] = gm[k];
  if (gl == 0) col[0] += 1;
  normalize<G, W>(col, gm, gl);
  montmul<G, W>(gm, rn, md.m, md.minv, gm, gl);  // (1 + m n) r^n
  if (live) store_limbs<W>(out + row * L, L, gl, gm);
}

// ---------------------------------------------------------------------- add
template <int L, int W>
__global__ __launch_bounds__(kWave) void k_add(Tables tb, int parties, uint64_t rows, Consts c, uint32_t* out) {
  constexpr int G = L / W;
  const int gl = threadIdx.x % G;
  bool live;
  const uint64_t row = my_row<G>(rows, &live);
  const Mod<W> md = mod_n2<W>(c, gl);
  uint32_t acc[W], b[W];
  load_limbs<W>(tb.ct[0] + row * L, L, gl, acc);
#pragma unroll 1
  for (int p = 1; p < parties; p++) {  // (acc R) b R^-1 = acc b
    load_limbs<W>(tb.ct[p] + row * L, L, gl, b);
    montmul<G, W>(acc, md.r2, md.m, md.minv, acc, gl);
    montmul<G, W>(acc, b, md.m, md.minv, acc, gl);
  }
  if (live) store_limbs<W>(out + row * L, L, gl, acc);
}

// ------------------------------------------------------------------ decrypt
template <int L, int W>
__global__ __launch_bounds__(kWave) void k_pow(const uint32_t* ct, uint64_t rows, Consts c, uint32_t* out) {
  constexpr int G = L / W;
  __shared__ uint32_t tab[(1 << kWindow) * kWave * W];
  const int gl = threadIdx.x % G;
  bool live;
  const uint64_t row = my_row<G>(rows, &live);
  const Mod<W> md = mod_n2<W>(c, gl);
  uint32_t x[W], b[W];
  load_limbs<W>(ct + row * L, L, gl, x);
  modexp<G, W>(x, md, c.lambda(), c.lambda_bits(), tab, x, gl);
#pragma unroll
  for (int k = 0; k < W; k++) b[k] = gl == 0 && k == 0;
  montmul<G, W>(x, b, md.m, md.minv, x, gl);
  if (live) store_limbs<W>(out + row * L, L, gl, x);
}

// x = c^lambda mod n^2 (rows of 2 LN limbs) -> ((x - 1) / n) mu mod n
template <int LN, int W>
__global__ __launch_bounds__(kWave) void k_lmu(const uint32_t* x, uint64_t rows, Consts c, uint32_t* out) {
  constexpr int G = LN / W;
  const int gl = threadIdx.x % G;
  bool live;
  const uint64_t row = my_row<G>(rows, &live);
  uint32_t nn[W], t[W], b[W], q[W];
  load_limbs<W>(c.n(), LN, gl, nn);
  load_limbs<W>(x + row * 2 * LN, LN, gl, t);
  // x == 0 (a ciphertext sharing every prime of n, 0 itself) is no power of
  // a unit: the quotient is then floor(-1 / n) = -1, as Python's // gives
  uint32_t any = 0;
  uint64_t col[W];
#pragma unroll
  for (int k = 0; k < W; k++) {
    any |= t[k];
    col[k] = (uint64_t)t[k] + 0xffffffffu;  // x - 1 mod 2^K
  }
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) any |= (uint32_t)__shfl_xor((int)any, off, G);
  normalize<G, W>(col, t, gl);
#pragma unroll
  for (int k = 0; k < W; k++) {
    b[k] = gl == 0 && k == 0;
    q[k] = 0;
  }
  montmul<G, W, true>(t, b, nn, c.minv_n(), t, gl, q);  // q = -(x - 1) / n mod 2^K
#pragma unroll
  for (int k = 0; k < W; k++) col[k] = (uint32_t)~q[k];
  if (gl == 0) col[0] += 1;
  normalize<G, W>(col, t, gl);
  if (!any) {
#pragma unroll
    for (int k = 0; k < W; k++) t[k] = nn[k] - (gl == 0 && k == 0);  // n - 1 (n is odd)
  }
  load_limbs<W>(c.mu_r(), LN, gl, b);
  montmul<G, W>(t, b, nn, c.minv_n(), t, gl);
  if (live) store_limbs<W>(out + row * LN, LN, gl, t);
}

// -------------------------------------------------------- encode and decode
struct Fields {
  uint64_t n, per_row;
  int bits, ln;
};

template <class T>
__device__ __forceinline__ uint64_t field_of(const T* x, uint64_t e, double w, double total, double bias,
                                             double expand, uint64_t limit, int bits, uint32_t* bad) {
  const double s = (double)x[e] * w / total + bias;
  if (s != s) {
    *bad |= SA_PPB_FLAG_NAN;
    return 0;
  }
  if (s < 0.0) {
    *bad |= SA_PPB_FLAG_NEGATIVE;
    return 0;
  }
  const double p = fabs(s) * expand;
  if (!(p < (double)(1ull << bits)) || (uint64_t)p > limit) {
    *bad |= SA_PPB_FLAG_RANGE;
    return 0;
  }
  return (uint64_t)p;
}

template <class T>
__global__ __launch_bounds__(256) void k_encode(const T* x, Fields f, double w, double total, double bias,
                                                double expand, uint64_t limit, uint32_t* plain, uint32_t* flags) {
  const uint64_t rows = (f.n + f.per_row - 1) / f.per_row;
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * f.ln) return;
  const uint64_t row = idx / f.ln;
  const int64_t bit0 = 32 * (int64_t)(idx % f.ln);
  const uint64_t left = f.n - row * f.per_row;
  const int64_t cnt = (int64_t)(left < f.per_row ? left : f.per_row);
  uint32_t limb = 0, bad = 0;
  // the first element of a row is its most significant field: position cnt - 1
  for (int64_t pos = bit0 / f.bits; pos <= (bit0 + 31) / f.bits && pos < cnt; pos++) {
    const uint64_t v = field_of<T>(x, row * f.per_row + (uint64_t)(cnt - 1 - pos), w, total, bias, expand, limit,
                                   f.bits, &bad);
    const int64_t shift = pos * f.bits - bit0;  // in -(bits - 1) .. 31
    limb |= shift >= 0 ? (uint32_t)(v << shift) : (uint32_t)(v >> -shift);
  }
  plain[idx] = limb;
  if (bad) atomicOr(flags, bad);
}

__global__ __launch_bounds__(256) void k_decode(const uint32_t* plain, Fields f, double expand, double c_bias,
                                                double* out) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= f.n) return;
  const uint64_t row = e / f.per_row, left = f.n - row * f.per_row;
  const uint64_t cnt = left < f.per_row ? left : f.per_row;
  const uint64_t bit = (cnt - 1 - e % f.per_row) * (uint64_t)f.bits;
  const uint32_t* p = plain + row * f.ln;
  const int l0 = (int)(bit >> 5), sh = (int)(bit & 31);
  auto limb = [&](int l) { return l < f.ln ? (uint64_t)p[l] : 0ull; };
  uint64_t v = (limb(l0) | (limb(l0 + 1) << 32)) >> sh;
  if (sh) v |= limb(l0 + 2) << (64 - sh);
  v &= (1ull << f.bits) - 1;
  out[e] = __ddiv_rn((double)v, expand) - c_bias;
}

// ------------------------------------------------------------------ entries
bool bad_ptr(const void* p, uintptr_t align) { return !p || ((uintptr_t)p & (align - 1)); }

int check_key_bits(int key_bits, const char* what) {
  switch (key_bits) {
    case 128: case 256: case 512: case 1024: case 2048:
      return SA_OK;
  }
  if (key_bits <= 0) {
    sa_set_error("%s: bad arguments (key_bits is positive)", what);
    return SA_ERR_ARG;
  }
  sa_set_error("%s: key size %d is not one of 128, 256, 512, 1024, 2048 (the host form takes any)", what, key_bits);
  return SA_ERR_UNSUPPORTED;
}

int check_fields(uint64_t n, int key_bits, int field_bits, const char* what, Fields* f) {
  int rc = check_key_bits(key_bits, what);
  if (rc != SA_OK) return rc;
  if (field_bits < 32 || field_bits > 63 || field_bits > key_bits - 1 || n >= (1ull << 40)) {
    sa_set_error("%s: field_bits in 32..63 and below key_bits, n < 2^40 are unsupported otherwise", what);
    return SA_ERR_UNSUPPORTED;
  }
  *f = Fields{n, (uint64_t)(key_bits / field_bits), field_bits, key_bits / 32};
  return SA_OK;
}

// the grid of a group-per-row kernel, or 0 when rows do not fit one
template <int G>
unsigned row_blocks(uint64_t rows) {
  const uint64_t b = (rows + kWave / G - 1) / (kWave / G);
  return b > 0x7fffffffull ? 0u : (unsigned)b;
}

// f(L, W) for the ciphertext width of key_bits: L = key_bits / 16 limbs
template <class F>
void dispatch_n2(int key_bits, F&& f) {
  switch (key_bits) {
    case 128: f(std::integral_constant<int, 8>(), std::integral_constant<int, 4>()); break;
    case 256: f(std::integral_constant<int, 16>(), std::integral_constant<int, 4>()); break;
    case 512: f(std::integral_constant<int, 32>(), std::integral_constant<int, 8>()); break;
    case 1024: f(std::integral_constant<int, 64>(), std::integral_constant<int, 8>()); break;
    default: f(std::integral_constant<int, 128>(), std::integral_constant<int, 8>()); break;
  }
}
// f(LN, W) for the plaintext width: LN = key_bits / 32 limbs
template <class F>
void dispatch_n(int key_bits, F&& f) {
  switch (key_bits) {
    case 128: f(std::integral_constant<int, 4>(), std::integral_constant<int, 4>()); break;
    case 256: f(std::integral_constant<int, 8>(), std::integral_constant<int, 4>()); break;
    case 512: f(std::integral_constant<int, 16>(), std::integral_constant<int, 4>()); break;
    case 1024: f(std::integral_constant<int, 32>(), std::integral_constant<int, 8>()); break;
    default: f(std::integral_constant<int, 64>(), std::integral_constant<int, 8>()); break;
  }
}

int check_rows(uint64_t rows, int key_bits, const uint32_t* consts, uint64_t n_consts, const char* what) {
  const int rc = check_key_bits(key_bits, what);
  if (rc != SA_OK) return rc;
  if (rows > 0x7fffffffull / 2 || n_consts != (uint64_t)consts_words(key_bits) || bad_ptr(consts, 4)) {
    sa_set_error("%s: bad arguments (rows < 2^30; consts: %d words, 4-byte aligned)", what, consts_words(key_bits));
    return SA_ERR_ARG;
  }
  return SA_OK;
}

}  // namespace

extern "C" int sa_ppb_consts_words(int key_bits) {
  const int rc = check_key_bits(key_bits, "sa_ppb_consts_words");
  return rc != SA_OK ? rc : consts_words(key_bits);
}

extern "C" int sa_ppb_encode(const void* x, int x_type, uint64_t n, double w, double total, int n_parties,
                             double bias, double expand, int key_bits, int field_bits, uint32_t* plain_out,
                             uint32_t* flags, void* stream) {
  const char* what = "sa_ppb_encode";
  int rc = sa::check_type(x_type, what);
  if (rc != SA_OK) return rc;
  if (n_parties < 1) {
    sa_set_error("%s: bad arguments (n_parties >= 1)", what);
    return SA_ERR_ARG;
  }
  Fields f;
  if ((rc = check_fields(n, key_bits, field_bits, what, &f)) != SA_OK) return rc;
  if (n == 0) return SA_OK;
  if (bad_ptr(x, x_type == SA_F32 ? 4 : 8) || bad_ptr(plain_out, 4) || bad_ptr(flags, 4)) {
    sa_set_error("%s: bad arguments (x, plain_out and flags are required, element-aligned)", what);
    return SA_ERR_ARG;
  }
  const uint64_t limit = ((1ull << field_bits) - 1) / (uint64_t)n_parties;
  const uint64_t limbs = (n + f.per_row - 1) / f.per_row * f.ln;
  int grid;
  if (!sa::tile_blocks(limbs, &grid)) {
    sa_set_error("%s: too many rows for one grid", what);
    return SA_ERR_ARG;
  }
  const dim3 g((unsigned)grid), b(256);
  hipStream_t s = (hipStream_t)stream;
  if (x_type == SA_F32)
    hipLaunchKernelGGL(k_encode<float>, g, b, 0, s, (const float*)x, f, w, total, bias, expand, limit, plain_out, flags);
  else if (x_type == SA_F64)
    hipLaunchKernelGGL(k_encode<double>, g, b, 0, s, (const double*)x, f, w, total, bias, expand, limit, plain_out,
                       flags);
  else
    hipLaunchKernelGGL(k_encode<int64_t>, g, b, 0, s, (const int64_t*)x, f, w, total, bias, expand, limit, plain_out,
                       flags);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_ppb_decode(const uint32_t* plain, uint64_t n, int n_parties, double bias, double expand,
                             int key_bits, int field_bits, double* out, void* stream) {
  const char* what = "sa_ppb_decode";
  Fields f;
  const int rc = check_fields(n, key_bits, field_bits, what, &f);
  if (rc != SA_OK) return rc;
  if (n == 0) return SA_OK;
  if (n_parties < 1 || bad_ptr(plain, 4) || bad_ptr(out, 8)) {
    sa_set_error("%s: bad arguments (n_parties >= 1; plain and out are required, element-aligned)", what);
    return SA_ERR_ARG;
  }
  int grid;
  if (!sa::tile_blocks(n, &grid)) {
    sa_set_error("%s: too many elements for one grid", what);
    return SA_ERR_ARG;
  }
  hipLaunchKernelGGL(k_decode, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, plain, f, expand,
                     (double)n_parties * bias, out);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_ppb_encrypt(const uint32_t* plain, uint64_t rows, int key_bits, const uint32_t* consts,
                              uint64_t n_consts, const uint32_t key[8], uint64_t nonce, uint32_t* ct_out,
                              uint32_t* flags, void* stream) {
  const char* what = "sa_ppb_encrypt";
  const int rc = check_rows(rows, key_bits, consts, n_consts, what);
  if (rc != SA_OK) return rc;
  if (rows == 0) return SA_OK;
  if (!key || bad_ptr(plain, 4) || bad_ptr(ct_out, 4) || bad_ptr(flags, 4)) {
    sa_set_error("%s: bad arguments (key, plain, ct_out and flags are required, 4-byte aligned)", what);
    return SA_ERR_ARG;
  }
  Key k;
  for (int i = 0; i < 8; i++) k.w[i] = key[i];
  const Consts c{consts, key_bits / 32};
  dispatch_n2(key_bits, [&](auto l, auto w) {
    constexpr int L = decltype(l)::value, W = decltype(w)::value;
    hipLaunchKernelGGL((k_encrypt<L, W>), dim3(row_blocks<L / W>(rows)), dim3(kWave), 0, (hipStream_t)stream, plain,
                       rows, c, k, nonce, ct_out, flags);
  });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_ppb_add(const uint32_t* const* cts, int n_parties, uint64_t rows, int key_bits,
                          const uint32_t* consts, uint64_t n_consts, uint32_t* out, void* stream) {
  const char* what = "sa_ppb_add";
  const int rc = check_rows(rows, key_bits, consts, n_consts, what);
  if (rc != SA_OK) return rc;
  if (n_parties < 1 || n_parties > SA_PPB_MAX_PARTIES || !cts) {
    sa_set_error("%s: bad arguments (1..%d parties, their table)", what, SA_PPB_MAX_PARTIES);
    return SA_ERR_ARG;
  }
  if (rows == 0) return SA_OK;
  Tables tb = {};
  for (int p = 0; p < n_parties; p++) {
    if (bad_ptr(cts[p], 4)) {
      sa_set_error("%s: bad arguments (party %d's ciphertexts are required, 4-byte aligned)", what, p);
      return SA_ERR_ARG;
    }
    tb.ct[p] = cts[p];
  }
  if (bad_ptr(out, 4)) {
    sa_set_error("%s: bad arguments (out is required, 4-byte aligned)", what);
    return SA_ERR_ARG;
  }
  const Consts c{consts, key_bits / 32};
  dispatch_n2(key_bits, [&](auto l, auto w) {
    constexpr int L = decltype(l)::value, W = decltype(w)::value;
    hipLaunchKernelGGL((k_add<L, W>), dim3(row_blocks<L / W>(rows)), dim3(kWave), 0, (hipStream_t)stream, tb,
                       n_parties, rows, c, out);
  });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_ppb_decrypt(const uint32_t* ct, uint64_t rows, int key_bits, const uint32_t* consts,
                              uint64_t n_consts, uint32_t* scratch, uint32_t* plain_out, void* stream) {
  const char* what = "sa_ppb_decrypt";
  const int rc = check_rows(rows, key_bits, consts, n_consts, what);
  if (rc != SA_OK) return rc;
  if (rows == 0) return SA_OK;
  if (bad_ptr(ct, 4) || bad_ptr(scratch, 4) || bad_ptr(plain_out, 4)) {
    sa_set_error("%s: bad arguments (ct, scratch and plain_out are required, 4-byte aligned)", what);
    return SA_ERR_ARG;
  }
  const Consts c{consts, key_bits / 32};
  dispatch_n2(key_bits, [&](auto l, auto w) {
    constexpr int L = decltype(l)::value, W = decltype(w)::value;
    hipLaunchKernelGGL((k_pow<L, W>), dim3(row_blocks<L / W>(rows)), dim3(kWave), 0, (hipStream_t)stream, ct, rows, c,
                       scratch);
  });
  SA_HIP_CHECK(hipGetLastError());
  dispatch_n(key_bits, [&](auto l, auto w) {
    constexpr int LN = decltype(l)::value, W = decltype(w)::value;
    hipLaunchKernelGGL((k_lmu<LN, W>), dim3(row_blocks<LN / W>(rows)), dim3(kWave), 0, (hipStream_t)stream,
                       (const uint32_t*)scratch, rows, c, plain_out);
  });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}
