// sa_stc.hip — sparse ternary compression (the reference's STCSparse,
// sfl/utils/compressor/sparse_compressor.py:142-179, with the error feedback
// of fed_stc.py:97-125 and the server's compress.py:28-42 around it) as one
// stream-ordered sequence of launches:
//
//   u       = (a - b) + r                      materialised once into res_out
//   masked  = the mask_num elements of smallest |u| (key = bits & 0x7f..f,
//             unsigned; equal keys: lower index first)
//   mu      = T(sum of the survivors' |u| in float64 / (n - mask_num))
//   sparse  = mu * sign(u_masked);  res' = u - sparse;  acc += sparse
//
// The threshold comes from a radix SELECT on the key (no sort): a histogram
// of one digit per pass, LDS-private per block, flushed with one integer
// atomic per non-empty bin, and a one-block scan that narrows (prefix, rank)
// in device memory.  Every wave owns a CONTIGUOUS index range, so wave order
// is index order: the ties at the threshold are counted per wave, scanned,
// and ranked in the last pass with ballots, which gives np.argsort(kind=
// "stable")'s "lower index first".  Nothing is allocated, copied to the host
// or synchronised; threshold, tie quota and mu never leave the device.
#include <hip/hip_runtime.h>

#include "sa_compress.h"

namespace sa {
namespace stc {

using namespace sa::elems;
using namespace sa::wave;  // the contiguous wave layout and the block scan
using namespace sa::entry;

// Key, State, the LDS histogram, k_init / k_hist / k_scan and the digit
// tables: the select, shared with sa_topk.hip
#include "sa_select.h"

constexpr size_t kOffHist = sizeof(State);
constexpr size_t kOffCnt = kOffHist + kMaxBins * sizeof(uint32_t);
constexpr size_t kOffSlots = kOffCnt + kMaxWaves * sizeof(uint32_t);
constexpr size_t kScratchBytes = kOffSlots + kMaxBlocks * sizeof(double);

// u = (a - b) + r -> u_out (may alias r), and the first digit's histogram.
template <class T>
__global__ void __launch_bounds__(kBlock) k_form(const T* __restrict__ a, const T* __restrict__ b, const T* r,
                                                 T* u_out, uint64_t n, uint64_t len, int vec, uint32_t* hist,
                                                 int shift, int nbins) {
  __shared__ __attribute__((aligned(16))) uint32_t h[kMaxBins * kCopies];
  const bool do_hist = hist != nullptr;
  if (do_hist) hist_clear(h);
  const Range w = wave_range(n, len);
  for (uint64_t t = w.lo; t < w.hi; t += kTile) {
    const uint64_t e0 = t + (uint64_t)w.lane * kEpl;
    const int cnt = lane_count(e0, w.hi);
    Elems<T> u = load_elems(a, e0, cnt, vec);
    if (b) {
      const Elems<T> y = load_elems(b, e0, cnt, vec);
#pragma unroll
      for (int j = 0; j < kEpl; j++) u.v[j] = u.v[j] - y.v[j];
    }
    if (r) {
      const Elems<T> y = load_elems(r, e0, cnt, vec);
#pragma unroll
      for (int j = 0; j < kEpl; j++) u.v[j] = u.v[j] + y.v[j];
    }
    store_elems(u_out, e0, cnt, vec, u);
    if (do_hist) {
#pragma unroll
      for (int j = 0; j < kEpl; j++) hist_add(h, (uint32_t)(Key<T>::of(u.v[j]) >> shift), j < cnt, w.lane);
    }
  }
  if (do_hist) hist_flush(h, hist, nbins);
}

// per wave: the ties at the threshold; per block: the float64 sum of the
// |u| above it (thread, wave, block: an order that depends on n only)
template <class T>
__global__ void __launch_bounds__(kBlock) k_count(const T* __restrict__ u, uint64_t n, uint64_t len, int vec,
                                                  const State* __restrict__ st, uint32_t* __restrict__ cnt,
                                                  double* __restrict__ slots) {
  typedef typename Key<T>::type K;
  __shared__ double wsum[kWaves];
  const K tau = (K)st->prefix;
  const Range w = wave_range(n, len);
  uint32_t ties = 0;
  double acc = 0.0;
  for (uint64_t t = w.lo; t < w.hi; t += 2 * kTile) {
    const uint64_t e0 = t + (uint64_t)w.lane * kEpl, e1 = e0 + kTile;
    const int c0 = lane_count(e0, w.hi), c1 = lane_count(e1, w.hi);
    const Elems<T> x0 = load_elems(u, e0, c0, vec);
    const Elems<T> x1 = load_elems(u, e1, c1, vec);
#pragma unroll
    for (int j = 0; j < kEpl; j++) {
      const K key = Key<T>::of(x0.v[j]);
      ties += (j < c0 && key == tau) ? 1u : 0u;
      if (j < c0 && key > tau) acc += (double)Key<T>::value(key);
    }
#pragma unroll
    for (int j = 0; j < kEpl; j++) {
      const K key = Key<T>::of(x1.v[j]);
      ties += (j < c1 && key == tau) ? 1u : 0u;
      if (j < c1 && key > tau) acc += (double)Key<T>::value(key);
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    ties += (uint32_t)__shfl_xor((int)ties, off, 64);
    acc += __shfl_xor(acc, off, 64);
  }
  if (w.lane == 0) {
    cnt[blockIdx.x * kWaves + (threadIdx.x >> 6)] = ties;
    wsum[threadIdx.x >> 6] = acc;
  }
  __syncthreads();
  if (threadIdx.x == 0) slots[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// One block: cnt -> exclusive prefix (each wave's first tie rank); the
// survivors' sum = the slots in a fixed order + the surviving ties, all of
// one magnitude; mu = T(S / (n - mask_num)).
template <class T>
__global__ void __launch_bounds__(kBlock) k_finish(uint32_t* cnt, int nwaves, const double* __restrict__ slots,
                                                   int nblocks, uint64_t kept, State* st, T* mu_out) {
  typedef typename Key<T>::type K;
  constexpr int PER = kMaxWaves / kBlock;
  __shared__ double dsum[kWaves];
  uint32_t c[PER], s = 0;
#pragma unroll
  for (int j = 0; j < PER; j++) {
    const int i = threadIdx.x * PER + j;
    c[j] = i < nwaves ? cnt[i] : 0u;
    s += c[j];
  }
  uint32_t total;
  uint32_t run = block_scan_incl(s, &total) - s;
#pragma unroll
  for (int j = 0; j < PER; j++) {
    const int i = threadIdx.x * PER + j;
    if (i < nwaves) cnt[i] = run;
    run += c[j];
  }
  double acc = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += kBlock) acc += slots[i];
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) dsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double S = (dsum[0] + dsum[1]) + (dsum[2] + dsum[3]);
    const uint32_t q = st->q;
    if (total > q) S += (double)(total - q) * (double)Key<T>::value((K)st->prefix);
    const T mu = kept == 0 ? T(0) : (T)(S / (double)kept);
    st->mu = (double)mu;
    if (mu_out) *mu_out = mu;
  }
}

template <class T>
__device__ __forceinline__ T sign_of(T x) {  // np.sign: -0 -> +0, NaN -> NaN
  return x > T(0) ? T(1) : (x < T(0) ? T(-1) : (x == T(0) ? T(0) : x));
}

// sparse = mu * sign(u_masked); res = u - sparse (in place on u); acc += sparse
template <class T>
__global__ void __launch_bounds__(kBlock) k_apply(T* u, T* __restrict__ sparse, T* __restrict__ accw, uint64_t n,
                                                  uint64_t len, int vec, const State* __restrict__ st,
                                                  const uint32_t* __restrict__ first_tie) {
  typedef typename Key<T>::type K;
  const K tau = (K)st->prefix;
  const uint32_t q = st->q;
  const T mu = (T)st->mu;
  const Range w = wave_range(n, len);
  uint32_t carry = first_tie[blockIdx.x * kWaves + (threadIdx.x >> 6)];
  const uint64_t below = ((uint64_t)1 << w.lane) - 1;
  for (uint64_t t = w.lo; t < w.hi; t += kTile) {
    const uint64_t e0 = t + (uint64_t)w.lane * kEpl;
    const int cnt = lane_count(e0, w.hi);
    Elems<T> x = load_elems(u, e0, cnt, vec);
    Elems<T> av;
    if (accw) av = load_elems(accw, e0, cnt, vec);
    K key[kEpl];
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < kEpl; j++) {
      key[j] = Key<T>::of(x.v[j]);
      c += (j < cnt && key[j] == tau) ? 1u : 0u;
    }
    // rank of this lane's first tie in index order (lane-major, then j)
    uint32_t rank = carry;
    if (__ballot(c != 0)) {
      const uint64_t b0 = __ballot(c & 1u), b1 = __ballot(c & 2u), b2 = __ballot(c & 4u);
      rank += (uint32_t)__popcll(b0 & below) + 2u * (uint32_t)__popcll(b1 & below) +
              4u * (uint32_t)__popcll(b2 & below);
      carry += (uint32_t)__popcll(b0) + 2u * (uint32_t)__popcll(b1) + 4u * (uint32_t)__popcll(b2);
    }
    Elems<T> sp;
#pragma unroll
    for (int j = 0; j < kEpl; j++) {
      bool masked = key[j] < tau;
      if (j < cnt && key[j] == tau) {
        masked = rank < q;
        rank++;
      }
      sp.v[j] = mu * sign_of(masked ? T(0) : x.v[j]);
      x.v[j] = x.v[j] - sp.v[j];
      if (accw) av.v[j] = av.v[j] + sp.v[j];
    }
    store_elems(sparse, e0, cnt, vec, sp);
    store_elems(u, e0, cnt, vec, x);
    if (accw) store_elems(accw, e0, cnt, vec, av);
  }
}


template <class T>
static int launch(const T* a, const T* b, const T* r, uint64_t n, uint64_t mask_num, T* sparse, T* res, T* acc,
                  T* mu_out, char* scratch, hipStream_t s) {
  State* st = reinterpret_cast<State*>(scratch);
  uint32_t* hist = reinterpret_cast<uint32_t*>(scratch + kOffHist);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(scratch + kOffCnt);
  double* slots = reinterpret_cast<double*>(scratch + kOffSlots);
  const Pass* passes = sizeof(T) == 4 ? kPasses32 : kPasses64;
  const int npass = sizeof(T) == 4 ? 3 : 6;

  // the grid is a function of n only: the survivors' sum has one order
  const auto [grid, nwaves, vec, len] = wave_grid(
      n, (uintptr_t)a | (uintptr_t)b | (uintptr_t)r | (uintptr_t)sparse | (uintptr_t)res | (uintptr_t)acc);

  // mask_num 0: threshold key 0 with quota 0 masks nothing; mask_num n: a
  // threshold above every key masks everything; neither needs the select
  const bool select = mask_num > 0 && mask_num < n;
  const uint64_t prefix0 = mask_num == n ? ~(uint64_t)0 : 0;
  hipLaunchKernelGGL(k_init, dim3(1), dim3(kBlock), 0, s, st, hist, prefix0,
                     (uint32_t)(select ? mask_num - 1 : 0));
  SA_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_form<T>, dim3(grid), dim3(kBlock), 0, s, a, b, r, res, n, len, vec,
                     select ? hist : (uint32_t*)nullptr, passes[0].shift, 1 << passes[0].bits);
  SA_HIP_CHECK(hipGetLastError());
  for (int p = 0; select && p < npass; p++) {
    if (p > 0) {
      hipLaunchKernelGGL(k_hist<T>, dim3(grid), dim3(kBlock), 0, s, (const T*)res, n, len, vec, (const State*)st,
                         hist, passes[p].shift, 1 << passes[p].bits);
      SA_HIP_CHECK(hipGetLastError());
    }
    if (passes[p].bits == 11)
      hipLaunchKernelGGL(k_scan<kMaxBins / kBlock>, dim3(1), dim3(kBlock), 0, s, hist, passes[p].shift,
                         p == npass - 1, st);
    else
      hipLaunchKernelGGL(k_scan<1024 / kBlock>, dim3(1), dim3(kBlock), 0, s, hist, passes[p].shift,
                         p == npass - 1, st);
    SA_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_count<T>, dim3(grid), dim3(kBlock), 0, s, (const T*)res, n, len, vec, (const State*)st, cnt,
                     slots);
  SA_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_finish<T>, dim3(1), dim3(kBlock), 0, s, cnt, nwaves, (const double*)slots, grid,
                     n - mask_num, st, mu_out);
  SA_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_apply<T>, dim3(grid), dim3(kBlock), 0, s, res, sparse, acc, n, len, vec, (const State*)st,
                     (const uint32_t*)cnt);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

}  // namespace stc
}  // namespace sa

using namespace sa::stc;

extern "C" int sa_stc_scratch_bytes(uint64_t n, int x_type) {
  int rc = check_float(x_type, "sa_stc_scratch_bytes", "x_type");
  if (rc == SA_OK) rc = check_n(n, 32, "sa_stc_scratch_bytes");
  return rc == SA_OK ? (int)kScratchBytes : rc;
}

extern "C" int sa_stc(const void* a, const void* b, const void* r, int x_type, uint64_t n, uint64_t mask_num,
                      void* sparse_out, void* res_out, void* acc_inout, void* mu_out, void* scratch,
                      void* stream) {
  int rc = check_float(x_type, "sa_stc", "x_type");
  if (rc == SA_OK) rc = check_n(n, 32, "sa_stc", " (ranks and counts are 32-bit)");
  if (rc != SA_OK) return rc;
  if (mask_num > n) {
    sa_set_error("sa_stc: mask_num exceeds n");
    return SA_ERR_ARG;
  }
  if (n == 0) return SA_OK;
  const uintptr_t esz = elem_size(x_type);
  const uintptr_t all = (uintptr_t)a | (uintptr_t)b | (uintptr_t)r | (uintptr_t)sparse_out | (uintptr_t)res_out |
                        (uintptr_t)acc_inout | (uintptr_t)mu_out;
  if (!a || !sparse_out || !res_out || !scratch || (all & (esz - 1)) || ((uintptr_t)scratch & 7)) {
    sa_set_error("sa_stc: bad arguments (a, sparse_out, res_out and scratch are required; element-aligned "
                 "vectors, 8-byte aligned scratch)");
    return SA_ERR_ARG;
  }
  if (a == res_out || (b && b == res_out) || sparse_out == res_out || sparse_out == a || sparse_out == b ||
      sparse_out == r || (acc_inout && (acc_inout == res_out || acc_inout == sparse_out || acc_inout == a))) {
    sa_set_error("sa_stc: only res_out may alias r");
    return SA_ERR_ARG;
  }
  return dispatch_float(x_type, [&](auto t) {
    typedef decltype(t) T;
    return launch((const T*)a, (const T*)b, (const T*)r, n, mask_num, (T*)sparse_out, (T*)res_out, (T*)acc_inout,
                  (T*)mu_out, (char*)scratch, (hipStream_t)stream);
  });
}
