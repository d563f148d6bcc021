// sa_quant.hip — the quantized compressors on the device (the reference's
// QuantizedZeroPoint, QuantizedLSTM and QuantizedFP at 8 bits,
// sfl/utils/compressor/quantized_compressor.py:65-228):
//
//   range    = min, max and max|x| of a tensor, NaN-propagating: every block
//              reduces its share to one partial in scratch, one block reduces
//              the partials (no atomics: the same input gives the same bits)
//   quant    = one streaming pass, x -> int8 / int16 codes
//   dequant  = one streaming pass, codes -> x
//
// The parameters between the two (scale and zero point, q and rqm, the fp8
// scale) are computed on the host from the three words of the range; the
// kernels only do the per-element arithmetic, every operation rounded in the
// data's type T (-ffp-contract=off; `/` is IEEE division, rint is
// round-half-to-even).
//
// Lane layout: a lane owns RUN consecutive elements ("a run"), consecutive
// lanes own consecutive runs, and a thread takes 16 / RUN runs a grid apart
// per iteration, so 16 elements are in flight per lane either way.  Encoding,
// a run is 16 elements: its codes are packed in registers and leave in ONE
// 16-byte store (two for int16), behind four (eight) 16-byte loads.  Decoding,
// a run is what fills ONE 16-byte store of floats (4 float32, 2 float64), its
// codes arriving in one load: consecutive lanes then write consecutive 16
// bytes.  Both were measured against the other choice (tools/quant_bench.py,
// DESIGN.md section 16).  A scalar head brings the code pointer to its
// vector's alignment; the elements after the last whole run are a scalar
// tail.  The float side takes 16-byte accesses when it is 16-byte aligned
// behind the head, element accesses with the same lane map otherwise.
#include <hip/hip_runtime.h>

#include "sa_runs.h"

namespace sa {
namespace quant {

using namespace sa::entry;
using namespace sa::runs;
using sa::wave::kBlock;
using sa::wave::kWaves;

// the grid's bound is sa_runs.h's kMaxBlocks; the fp8 decoder, which the VALU
// bounds, wants twice as many waves
constexpr int kFp8DecodeBlocks = 2 * kMaxBlocks;

// scratch of the range: per block min, max and a NaN mark, as three T
constexpr size_t kScratchBytes = (size_t)kMaxBlocks * 3 * sizeof(double);

__device__ __forceinline__ float t_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double t_min(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ float t_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double t_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float t_rint(float a) { return rintf(a); }
__device__ __forceinline__ double t_rint(double a) { return rint(a); }
__device__ __forceinline__ float t_frexp(float a, int* e) { return frexpf(a, e); }
__device__ __forceinline__ double t_frexp(double a, int* e) { return frexp(a, e); }
__device__ __forceinline__ float t_ldexp(float a, int e) { return ldexpf(a, e); }
__device__ __forceinline__ double t_ldexp(double a, int e) { return ldexp(a, e); }
__device__ __forceinline__ float t_shfl(float a, int off) { return __shfl_xor(a, off, 64); }
__device__ __forceinline__ double t_shfl(double a, int off) { return __shfl_xor(a, off, 64); }

template <class T>
struct Lim;
template <>
struct Lim<float> {
  static __device__ __forceinline__ float inf() { return __uint_as_float(0x7f800000u); }
  static __device__ __forceinline__ float nan() { return __uint_as_float(0x7fc00000u); }
};
template <>
struct Lim<double> {
  static __device__ __forceinline__ double inf() { return __longlong_as_double(0x7ff0000000000000ll); }
  static __device__ __forceinline__ double nan() { return __longlong_as_double(0x7ff8000000000000ll); }
};

// --- the per-element arithmetic ------------------------------------------------

// code = int(rint(clip(x / scale + z, lo, hi)))
template <class T>
struct ZeroPoint {
  T scale, z, lo, hi;
  __device__ __forceinline__ int32_t enc(T x) const {
    const T v = x / scale + z;
    return (int32_t)t_rint(t_min(t_max(v, lo), hi));
  }
  __device__ __forceinline__ T dec(int32_t c) const { return ((T)c - z) * scale; }
};

// code = sat(rint(q * x) - rqm); lo and hi are the storage range
template <class T>
struct Lstm {
  T q, rqm, lo, hi;
  __device__ __forceinline__ int32_t enc(T x) const {
    const T v = t_rint(q * x) - rqm;
    return (int32_t)t_min(t_max(v, lo), hi);
  }
  __device__ __forceinline__ T dec(int32_t c) const { return ((T)c + rqm) / q; }
};

// sign | exponent field | mantissa field, qm == mant_len carrying into the exponent
template <class T, int mant_len, int exp_offset>
struct Fp8 {
  T scale;
  __device__ __forceinline__ int32_t enc(T x) const {
    int e;
    const T m = t_frexp((x < T(0) ? -x : x) * scale, &e);
    const int qe = e > -exp_offset ? e + exp_offset : 0;
    const T qm = t_rint((T(2) * m - T(1)) * (T)mant_len);
    const int s = x > T(0) ? 1 : (x < T(0) ? -1 : 0);
    return s * (qe * mant_len + (int)qm);
  }
  __device__ __forceinline__ T dec(int32_t code) const {
    const uint32_t c = code < 0 ? -code : code;  // int32: -128 is 128
    const T mant = ((T)(c % mant_len) / (T)mant_len + T(1)) / T(2);
    const T s = code > 0 ? T(1) : (code < 0 ? T(-1) : T(0));
    return s * t_ldexp(mant, (int)(c / mant_len) - exp_offset) / scale;
  }
};

// --- the streaming passes -----------------------------------------------------

// elements [0, head) and [head + nruns * kRun, n) are the scalar head and tail
// (both shorter than 16), taken by the first threads of block 0
template <class T, int QB, class Op, int kRun>
__global__ void __launch_bounds__(kBlock) k_quant(const T* __restrict__ x, uint64_t n, uint32_t head, uint64_t nruns,
                                                  int vec, Op op, void* __restrict__ q) {
  constexpr int kUnroll = 16 / kRun;
  const uint64_t nthreads = (uint64_t)gridDim.x * kBlock;
  const T* xb = x + head;
  char* qb = reinterpret_cast<char*>(q) + (uint64_t)head * QB;
  for (uint64_t r0 = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r0 < nruns; r0 += nthreads * kUnroll) {
    T v[kUnroll][kRun];
#pragma unroll
    for (int u = 0; u < kUnroll; u++) {
      const uint64_t r = r0 + u * nthreads;
      if (r < nruns) load_run<T, kRun>(xb + r * kRun, v[u], vec);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; u++) {
      const uint64_t r = r0 + u * nthreads;
      if (r < nruns) {
        int32_t c[kRun];
#pragma unroll
        for (int j = 0; j < kRun; j++) c[j] = op.enc(v[u][j]);
        Codes<QB, kRun> out;
        out.pack(c);
        out.store(qb + r * kRun * QB);
      }
    }
  }
  if (blockIdx.x == 0) {
    const uint64_t t = threadIdx.x, tail0 = head + nruns * kRun;
    if (t < head) store_code<QB>(q, t, op.enc(x[t]));
    if (tail0 + t < n) store_code<QB>(q, tail0 + t, op.enc(x[tail0 + t]));
  }
}

template <class T, int QB, class Op, int kRun>
__global__ void __launch_bounds__(kBlock) k_dequant(const void* __restrict__ q, uint64_t n, uint32_t head,
                                                    uint64_t nruns, int vec, Op op, T* __restrict__ out) {
  constexpr int kUnroll = 16 / kRun;
  const uint64_t nthreads = (uint64_t)gridDim.x * kBlock;
  T* ob = out + head;
  const char* qb = reinterpret_cast<const char*>(q) + (uint64_t)head * QB;
  for (uint64_t r0 = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r0 < nruns; r0 += nthreads * kUnroll) {
    Codes<QB, kRun> in[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; u++) {
      const uint64_t r = r0 + u * nthreads;
      if (r < nruns) in[u].load(qb + r * kRun * QB);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; u++) {
      const uint64_t r = r0 + u * nthreads;
      if (r < nruns) {
        int32_t c[kRun];
        in[u].unpack(c);
        T v[kRun];
#pragma unroll
        for (int j = 0; j < kRun; j++) v[j] = op.dec(c[j]);
        store_run<T, kRun>(ob + r * kRun, v, vec);
      }
    }
  }
  if (blockIdx.x == 0) {
    const uint64_t t = threadIdx.x, tail0 = head + nruns * kRun;
    if (t < head) out[t] = op.dec(load_code<QB>(q, t));
    if (tail0 + t < n) out[tail0 + t] = op.dec(load_code<QB>(q, tail0 + t));
  }
}

// --- the range ------------------------------------------------------------------

template <class T>
struct MinMax {
  T mn, mx;
  int nan;
  __device__ __forceinline__ void take(T x) {
    mn = t_min(mn, x), mx = t_max(mx, x);  // fmin / fmax skip a NaN: it is marked apart
    nan |= x != x;
  }
  __device__ __forceinline__ void merge(const MinMax& o) {
    mn = t_min(mn, o.mn), mx = t_max(mx, o.mx), nan |= o.nan;
  }
};

template <class T>
__device__ __forceinline__ MinMax<T> block_minmax(MinMax<T> a) {
  __shared__ T smn[kWaves], smx[kWaves];
  __shared__ int snan[kWaves];
  for (int off = 32; off > 0; off >>= 1) {
    MinMax<T> o;
    o.mn = t_shfl(a.mn, off), o.mx = t_shfl(a.mx, off), o.nan = __shfl_xor(a.nan, off, 64);
    a.merge(o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) smn[wave] = a.mn, smx[wave] = a.mx, snan[wave] = a.nan;
  __syncthreads();
  MinMax<T> r = {smn[0], smx[0], snan[0]};
  for (int i = 1; i < kWaves; i++) r.merge(MinMax<T>{smn[i], smx[i], snan[i]});
  return r;
}

// stage 1: block b's share of x -> part[3 b .. 3 b + 2] = (min, max, NaN mark).
// x + head is 16-byte aligned; a vector is 16 / sizeof(T) elements.
template <class T>
__global__ void __launch_bounds__(kBlock) k_range(const T* __restrict__ x, uint64_t n, uint32_t head, uint64_t nvecs,
                                                  T* __restrict__ part) {
  constexpr int V = 16 / sizeof(T), U = 4;
  const uint64_t nthreads = (uint64_t)gridDim.x * kBlock;
  const T* xb = x + head;
  MinMax<T> a = {Lim<T>::inf(), -Lim<T>::inf(), 0};
  for (uint64_t r0 = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r0 < nvecs; r0 += nthreads * U) {
    T v[U][V];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint64_t r = r0 + u * nthreads;
      if (r < nvecs) load_run<T, V>(xb + r * V, v[u], true);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint64_t r = r0 + u * nthreads;
      if (r < nvecs) {
#pragma unroll
        for (int j = 0; j < V; j++) a.take(v[u][j]);
      }
    }
  }
  if (blockIdx.x == 0) {
    const uint64_t t = threadIdx.x, tail0 = head + nvecs * V;
    if (t < head) a.take(x[t]);
    if (tail0 + t < n) a.take(x[tail0 + t]);
  }
  a = block_minmax(a);
  if (threadIdx.x == 0) {
    part[3 * blockIdx.x] = a.mn, part[3 * blockIdx.x + 1] = a.mx, part[3 * blockIdx.x + 2] = a.nan ? T(1) : T(0);
  }
}

// stage 2, one block: the partials -> out = (min, max, max|x|); NaN if any
// element was one.  max|x| = max(-min, max).  No element: (inf, -inf, 0).
template <class T>
__global__ void __launch_bounds__(kBlock) k_range_final(const T* __restrict__ part, int nparts, T* __restrict__ out) {
  MinMax<T> a = {Lim<T>::inf(), -Lim<T>::inf(), 0};
  for (int i = threadIdx.x; i < nparts; i += kBlock)
    a.merge(MinMax<T>{part[3 * i], part[3 * i + 1], part[3 * i + 2] != T(0)});
  a = block_minmax(a);
  if (threadIdx.x == 0) {
    const T nan = Lim<T>::nan();
    out[0] = a.nan ? nan : a.mn;
    out[1] = a.nan ? nan : a.mx;
    out[2] = a.nan ? nan : t_max(T(0), t_max(-a.mn, a.mx));
  }
}

// --- checks and launches (sa_runs.h: the plan of a pass, the vectors' check) ---

static int check_mode(int mode, const char* what) {
  if (mode != SA_QUANT_ZERO_POINT && mode != SA_QUANT_LSTM) {
    sa_set_error("%s: mode must be SA_QUANT_ZERO_POINT or SA_QUANT_LSTM", what);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

static int check_clamp(int qmin, int qmax, int q_bytes, const char* what) {
  const int lim = q_bytes == 1 ? 128 : 32768;
  if (qmin >= qmax || qmin < -lim || qmax > lim - 1) {
    sa_set_error("%s: [qmin, qmax] must be a range inside the codes' storage type", what);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

static int check_fp8(int mant_len, int exp_offset, const char* what) {
  if (!((mant_len == 8 && exp_offset == 6) || (mant_len == 4 && exp_offset == 14))) {
    sa_set_error("%s: (mant_len, exp_offset) must be (8, 6) for E4M3 or (4, 14) for E5M2", what);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

template <class T, int QB, class Op>
static void launch_quant(const void* x, uint64_t n, const Op& op, void* q, hipStream_t s) {
  const Plan p = plan_of(n, q, Codes<QB, kEncRun>::kAlign, QB, x, sizeof(T), kEncRun, 16 / kEncRun);
  hipLaunchKernelGGL((k_quant<T, QB, Op, kEncRun>), dim3(p.grid), dim3(kBlock), 0, s, (const T*)x, n, p.head, p.nruns, p.vec,
                     op, q);
}

template <class T, int QB, class Op>
static void launch_dequant(const void* q, uint64_t n, const Op& op, void* out, hipStream_t s,
                           int max_blocks = kMaxBlocks) {
  constexpr int kRun = kDecRun<T>;
  const Plan p = plan_of(n, q, Codes<QB, kRun>::kAlign, QB, out, sizeof(T), kRun, 16 / kRun, max_blocks);
  hipLaunchKernelGGL((k_dequant<T, QB, Op, kRun>), dim3(p.grid), dim3(kBlock), 0, s, q, n, p.head, p.nruns, p.vec, op,
                     (T*)out);
}

template <class T>
static void launch_affine(bool encode, const void* x, uint64_t n, int mode, double p0, double p1, int qmin, int qmax,
                          void* q, int q_bytes, hipStream_t s) {
  if (mode == SA_QUANT_ZERO_POINT) {
    const ZeroPoint<T> op = {(T)p0, (T)p1, (T)qmin, (T)qmax};
    if (encode)
      q_bytes == 1 ? launch_quant<T, 1>(x, n, op, q, s) : launch_quant<T, 2>(x, n, op, q, s);
    else
      q_bytes == 1 ? launch_dequant<T, 1>(q, n, op, (void*)x, s) : launch_dequant<T, 2>(q, n, op, (void*)x, s);
  } else {
    const Lstm<T> op = {(T)p0, (T)p1, (T)qmin, (T)qmax};
    if (encode)
      q_bytes == 1 ? launch_quant<T, 1>(x, n, op, q, s) : launch_quant<T, 2>(x, n, op, q, s);
    else
      q_bytes == 1 ? launch_dequant<T, 1>(q, n, op, (void*)x, s) : launch_dequant<T, 2>(q, n, op, (void*)x, s);
  }
}

// the two formats check_fp8 admits, as compile-time constants: the field
// arithmetic is shifts and masks, the divisions by mant_len and 2 exact
template <class T>
static void launch_fp8(bool encode, const void* x, uint64_t n, double scale, int mant_len, void* q, hipStream_t s) {
  const Fp8<T, 8, 6> e4m3 = {(T)scale};
  const Fp8<T, 4, 14> e5m2 = {(T)scale};
  if (encode)
    mant_len == 8 ? launch_quant<T, 1>(x, n, e4m3, q, s) : launch_quant<T, 1>(x, n, e5m2, q, s);
  else
    mant_len == 8 ? launch_dequant<T, 1>(q, n, e4m3, (void*)x, s, kFp8DecodeBlocks)
                  : launch_dequant<T, 1>(q, n, e5m2, (void*)x, s, kFp8DecodeBlocks);
}

template <class T>
static void launch_range(const void* x, uint64_t n, void* scratch, void* out, hipStream_t s) {
  constexpr int V = 16 / sizeof(T), U = 4;
  const Plan p = plan_of(n, x, 16, sizeof(T), x, sizeof(T), V, U);
  hipLaunchKernelGGL(k_range<T>, dim3(p.grid), dim3(kBlock), 0, s, (const T*)x, n, p.head, p.nruns, (T*)scratch);
  hipLaunchKernelGGL(k_range_final<T>, dim3(1), dim3(kBlock), 0, s, (const T*)scratch, p.grid, (T*)out);
}

}  // namespace quant
}  // namespace sa

using namespace sa::quant;

extern "C" int sa_quant_scratch_bytes(uint64_t n, int x_type) {
  const int rc = check_float_n(x_type, n, 32, "sa_quant_scratch_bytes");
  return rc == SA_OK ? (int)kScratchBytes : rc;
}

extern "C" int sa_quant_range(const void* x, int x_type, uint64_t n, void* scratch, void* out3, void* stream) {
  const int rc = check_float_n(x_type, n, 32, "sa_quant_range");
  if (rc != SA_OK) return rc;
  const uintptr_t esz = elem_size(x_type);
  if ((n && !x) || misaligned(x, esz) || !scratch || misaligned(scratch, 8) || !out3 || misaligned(out3, esz)) {
    sa_set_error("sa_quant_range: bad arguments (x, scratch and out3 are required; element-aligned x and out3, "
                 "8-byte aligned scratch)");
    return SA_ERR_ARG;
  }
  dispatch_float(x_type, [&](auto t) { launch_range<decltype(t)>(x, n, scratch, out3, (hipStream_t)stream); });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_quant_affine(const void* x, int x_type, uint64_t n, int mode, double p0, double p1, int qmin,
                               int qmax, void* q_out, int q_bytes, void* stream) {
  int rc = check_float_n(x_type, n, 32, "sa_quant_affine");
  if (rc == SA_OK) rc = check_vectors(x, elem_size(x_type), q_out, q_bytes, n, "sa_quant_affine");
  if (rc == SA_OK) rc = check_mode(mode, "sa_quant_affine");
  if (rc == SA_OK) rc = check_clamp(qmin, qmax, q_bytes, "sa_quant_affine");
  if (rc != SA_OK) return rc;
  if (n == 0) return SA_OK;
  dispatch_float(x_type, [&](auto t) {
    launch_affine<decltype(t)>(true, x, n, mode, p0, p1, qmin, qmax, q_out, q_bytes, (hipStream_t)stream);
  });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_dequant_affine(const void* q, int q_bytes, uint64_t n, int mode, double p0, double p1, int x_type,
                                 void* out, void* stream) {
  int rc = check_float_n(x_type, n, 32, "sa_dequant_affine");
  if (rc == SA_OK) rc = check_vectors(out, elem_size(x_type), q, q_bytes, n, "sa_dequant_affine");
  if (rc == SA_OK) rc = check_mode(mode, "sa_dequant_affine");
  if (rc != SA_OK) return rc;
  if (n == 0) return SA_OK;
  dispatch_float(x_type, [&](auto t) {
    launch_affine<decltype(t)>(false, out, n, mode, p0, p1, 0, 0, (void*)q, q_bytes, (hipStream_t)stream);
  });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_quant_fp8(const void* x, int x_type, uint64_t n, double scale, int mant_len, int exp_offset,
                            void* q_out, void* stream) {
  int rc = check_float_n(x_type, n, 32, "sa_quant_fp8");
  if (rc == SA_OK) rc = check_vectors(x, elem_size(x_type), q_out, 1, n, "sa_quant_fp8");
  if (rc == SA_OK) rc = check_fp8(mant_len, exp_offset, "sa_quant_fp8");
  if (rc != SA_OK) return rc;
  if (n == 0) return SA_OK;
  dispatch_float(x_type,
                 [&](auto t) { launch_fp8<decltype(t)>(true, x, n, scale, mant_len, q_out, (hipStream_t)stream); });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_dequant_fp8(const void* q, uint64_t n, double scale, int mant_len, int exp_offset, int x_type,
                              void* out, void* stream) {
  int rc = check_float_n(x_type, n, 32, "sa_dequant_fp8");
  if (rc == SA_OK) rc = check_vectors(out, elem_size(x_type), q, 1, n, "sa_dequant_fp8");
  if (rc == SA_OK) rc = check_fp8(mant_len, exp_offset, "sa_dequant_fp8");
  if (rc != SA_OK) return rc;
  if (n == 0) return SA_OK;
  dispatch_float(x_type, [&](auto t) {
    launch_fp8<decltype(t)>(false, out, n, scale, mant_len, (void*)q, (hipStream_t)stream);
  });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}
