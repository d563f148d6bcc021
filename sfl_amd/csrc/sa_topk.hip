// sa_topk.hip — top-k sparsification on the device (the reference's TopkSparse
// and RandomSparse, sfl/utils/compressor/sparse_compressor.py:97-139) as a
// SELECT followed by a COMPACTION; the result never becomes a dense
// intermediate:
//
//   kept    = the k elements of largest key (key = bits & 0x7f..f, unsigned;
//             equal keys at the threshold: the HIGHER indices are kept, the
//             complement of what sa_stc masks at mask_num = n - k)
//   payload = (index, data): the kept flat positions, strictly ascending, and
//             x at those positions, bit for bit
//
// sa_topk_select is sa_stc's radix select (sa_select.h) for rank n - k - 1,
// the largest dropped key, then one counting pass (per wave: the keys above
// the threshold and the ties at it) and one block that turns the tie counts
// into each wave's first tie rank and the kept counts into exclusive output
// offsets.  sa_topk_fill is sa_coo's ballot-rank compaction with the ties
// ranked as sa_stc's last pass ranks them.  Every wave owns a CONTIGUOUS index
// range, so wave order is index order: no atomics beyond the histogram's
// integer adds, no sort.  Nothing is allocated, copied to the host or
// synchronised; k is known on the host, so not even a count is read back.
//
// RandomSparse selects on keys of its own: sa_topk_random_keys writes 63 bits
// of a Philox4x32-10 stream per element, and the k largest are kept by the
// same two entries with x as a second vector.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "sa_compress.h"
#include "sa_philox.h"

namespace sa {
namespace topk {

using namespace sa::elems;
using namespace sa::wave;  // the contiguous wave layout and the block scan
using namespace sa::entry;

// Key, State, the LDS histogram, k_init / k_hist / k_scan and the digit
// tables: the select, shared with sa_stc.hip
#include "sa_select.h"

// scratch: the select's state and histogram; per wave its ties (after
// k_offsets: its first tie rank) and its keys above the threshold (after
// k_offsets: its first output rank); the number of kept entries
constexpr size_t kOffHist = sizeof(State);
constexpr size_t kOffTies = kOffHist + kMaxBins * sizeof(uint32_t);
constexpr size_t kOffKept = kOffTies + kMaxWaves * sizeof(uint32_t);
constexpr size_t kOffTotal = kOffKept + kMaxWaves * sizeof(uint32_t);
constexpr size_t kScratchBytes = kOffTotal + 2 * sizeof(uint32_t);
static_assert(kScratchBytes % 8 == 0, "scratch layout");

// per wave: the ties at the threshold and the keys above it
template <class T>
__global__ void __launch_bounds__(kBlock) k_count(const T* __restrict__ keys, uint64_t n, uint64_t len, int vec,
                                                  const State* __restrict__ st, uint32_t* __restrict__ ties_out,
                                                  uint32_t* __restrict__ above_out) {
  typedef typename Key<T>::type K;
  const K tau = (K)st->prefix;
  const Range w = wave_range(n, len);
  uint32_t ties = 0, above = 0;
  for (uint64_t t = w.lo; t < w.hi; t += 2 * kTile) {
    const uint64_t e0 = t + (uint64_t)w.lane * kEpl, e1 = e0 + kTile;
    const int c0 = lane_count(e0, w.hi), c1 = lane_count(e1, w.hi);
    const Elems<T> x0 = load_elems(keys, e0, c0, vec);
    const Elems<T> x1 = load_elems(keys, e1, c1, vec);
#pragma unroll
    for (int j = 0; j < kEpl; j++) {
      const K k0 = Key<T>::of(x0.v[j]), k1 = Key<T>::of(x1.v[j]);
      ties += (j < c0 && k0 == tau) ? 1u : 0u;
      above += (j < c0 && k0 > tau) ? 1u : 0u;
      ties += (j < c1 && k1 == tau) ? 1u : 0u;
      above += (j < c1 && k1 > tau) ? 1u : 0u;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    ties += (uint32_t)__shfl_xor((int)ties, off, 64);
    above += (uint32_t)__shfl_xor((int)above, off, 64);
  }
  if (w.lane == 0) {
    ties_out[blockIdx.x * kWaves + (threadIdx.x >> 6)] = ties;
    above_out[blockIdx.x * kWaves + (threadIdx.x >> 6)] = above;
  }
}

// One block: ties -> exclusive prefix (each wave's first tie rank); a wave
// keeps its keys above the threshold and its ties of rank >= q; kept ->
// exclusive prefix (each wave's first output rank), the total into *total.
__global__ void __launch_bounds__(kBlock) k_offsets(uint32_t* ties, uint32_t* kept, int nwaves,
                                                    const State* __restrict__ st, uint32_t* __restrict__ total_out) {
  constexpr int PER = kMaxWaves / kBlock;
  const uint32_t q = st->q;
  uint32_t c[PER], s = 0;
#pragma unroll
  for (int j = 0; j < PER; j++) {
    const int i = threadIdx.x * PER + j;
    c[j] = i < nwaves ? ties[i] : 0u;
    s += c[j];
  }
  uint32_t total;
  uint32_t run = block_scan_incl(s, &total) - s;
  uint32_t a[PER], sk = 0;
#pragma unroll
  for (int j = 0; j < PER; j++) {
    const int i = threadIdx.x * PER + j;
    const uint32_t lo = run > q ? run : q, hi = run + c[j];  // the wave's tie ranks [run, hi), kept from q on
    if (i < nwaves) ties[i] = run;
    a[j] = i < nwaves ? kept[i] + (hi > lo ? hi - lo : 0u) : 0u;
    sk += a[j];
    run = hi;
  }
  __syncthreads();  // the scan's LDS words: every thread has read the first scan's
  run = block_scan_incl(sk, &total) - sk;
#pragma unroll
  for (int j = 0; j < PER; j++) {
    const int i = threadIdx.x * PER + j;
    if (i < nwaves) kept[i] = run;
    run += a[j];
  }
  if (threadIdx.x == 0) *total_out = total;
}

// The compaction: an entry's rank = its wave's first output rank + the
// earlier tiles' count + the ballot prefix of the lane counts (lane-major,
// then j: index order).  A tie's rank among the ties comes from the same
// three ballots, as in sa_stc's k_apply; ties of rank >= q are kept.
// x == keys (one element type): one load serves both.
template <class KT, class XT>
__global__ void __launch_bounds__(kBlock) k_fill(const KT* keys, const XT* x, uint64_t n, uint64_t len, int vec,
                                                 const State* __restrict__ st,
                                                 const uint32_t* __restrict__ first_tie,
                                                 const uint32_t* __restrict__ first_out,
                                                 const uint32_t* __restrict__ total, int32_t* __restrict__ index_out,
                                                 XT* __restrict__ data_out, uint32_t cap, uint32_t* flag) {
  typedef typename Key<KT>::type K;
  if (blockIdx.x == 0 && threadIdx.x == 0 && *total != cap) atomicOr(&flag[0], (uint32_t)SA_COO_BAD_COUNT);
  const K tau = (K)st->prefix;
  const uint32_t q = st->q;
  const Range w = wave_range(n, len);
  uint32_t tcarry = first_tie[blockIdx.x * kWaves + (threadIdx.x >> 6)];
  uint32_t ocarry = first_out[blockIdx.x * kWaves + (threadIdx.x >> 6)];
  const uint64_t below = ((uint64_t)1 << w.lane) - 1;
  for (uint64_t t = w.lo; t < w.hi; t += kTile) {
    const uint64_t e0 = t + (uint64_t)w.lane * kEpl;
    const int cnt = lane_count(e0, w.hi);
    const Elems<KT> kv = load_elems(keys, e0, cnt, vec);
    K key[kEpl];
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < kEpl; j++) {
      key[j] = Key<KT>::of(kv.v[j]);
      c += (j < cnt && key[j] == tau) ? 1u : 0u;
    }
    // rank of this lane's first tie in index order (lane-major, then j)
    uint32_t trank = tcarry;
    if (__ballot(c != 0)) {
      const uint64_t b0 = __ballot(c & 1u), b1 = __ballot(c & 2u), b2 = __ballot(c & 4u);
      trank += (uint32_t)__popcll(b0 & below) + 2u * (uint32_t)__popcll(b1 & below) +
               4u * (uint32_t)__popcll(b2 & below);
      tcarry += (uint32_t)__popcll(b0) + 2u * (uint32_t)__popcll(b1) + 4u * (uint32_t)__popcll(b2);
    }
    bool keep[kEpl];
    uint32_t kc = 0;
#pragma unroll
    for (int j = 0; j < kEpl; j++) {
      keep[j] = j < cnt && key[j] > tau;
      if (j < cnt && key[j] == tau) {
        keep[j] = trank >= q;
        trank++;
      }
      kc += keep[j] ? 1u : 0u;
    }
    if (__ballot(kc != 0) == 0) continue;  // wave-uniform
    const uint64_t b0 = __ballot(kc & 1u), b1 = __ballot(kc & 2u), b2 = __ballot(kc & 4u);
    uint32_t rank = ocarry + (uint32_t)__popcll(b0 & below) + 2u * (uint32_t)__popcll(b1 & below) +
                    4u * (uint32_t)__popcll(b2 & below);
    ocarry += (uint32_t)__popcll(b0) + 2u * (uint32_t)__popcll(b1) + 4u * (uint32_t)__popcll(b2);
    Elems<XT> v;
    if constexpr (std::is_same<KT, XT>::value) {
      if ((const void*)x == (const void*)keys)  // kernel-uniform
        v = kv;
      else
        v = load_elems(x, e0, cnt, vec);
    } else {
      v = load_elems(x, e0, cnt, vec);
    }
#pragma unroll
    for (int j = 0; j < kEpl; j++) {
      if (keep[j]) {
        if (rank < cap) {
          index_out[rank] = (int32_t)(e0 + j);
          data_out[rank] = v.v[j];
        }
        rank++;
      }
    }
  }
}

// --- RandomSparse's keys ---------------------------------------------------------
// element e: words 2e and 2e + 1 of the Philox stream under `seed`, i.e. the
// low or the high pair of counter block e >> 1; key = (hi:lo) >> 1, 63 bits,
// so the word read as a float64 has its sign bit clear

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

__host__ __device__ inline uint64_t key63(uint32_t lo, uint32_t hi) { return (((uint64_t)hi << 32) | lo) >> 1; }

// one counter block, two keys, per thread and step
__global__ void __launch_bounds__(kBlock) k_random_keys(uint64_t seed, uint64_t n, int vec,
                                                        uint64_t* __restrict__ out) {
  const uint64_t nblk = (n + 1) >> 1;
  for (uint64_t b = (uint64_t)blockIdx.x * kBlock + threadIdx.x; b < nblk; b += (uint64_t)gridDim.x * kBlock) {
    uint32_t c[4];
    philox_block(seed, b, c);
    const uint64_t k0 = key63(c[0], c[1]), k1 = key63(c[2], c[3]), e = 2 * b;
    if (vec && e + 1 < n) {
      u64x2 t;
      t.x = k0, t.y = k1;
      *reinterpret_cast<u64x2*>(out + e) = t;
    } else {
      out[e] = k0;
      if (e + 1 < n) out[e + 1] = k1;
    }
  }
}

static int check_type_n(int key_type, uint64_t n, const char* what) {
  const int rc = check_float(key_type, what, "key_type");
  return rc != SA_OK ? rc : check_n(n, 31, what, " (the flat index is int32)");
}

static int check_k(uint64_t k, uint64_t n, const char* what) {
  if (k > n) {
    sa_set_error("%s: k exceeds n", what);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

// do [a, a + abytes) and [b, b + bbytes) share a byte?
static bool overlap(const void* a, uint64_t abytes, const void* b, uint64_t bbytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && abytes && bbytes && x < y + bbytes && y < x + abytes;
}

template <class T>
static int launch_select(const T* keys, uint64_t n, uint64_t k, char* scratch, hipStream_t s) {
  State* st = reinterpret_cast<State*>(scratch);
  uint32_t* hist = reinterpret_cast<uint32_t*>(scratch + kOffHist);
  uint32_t* ties = reinterpret_cast<uint32_t*>(scratch + kOffTies);
  uint32_t* kept = reinterpret_cast<uint32_t*>(scratch + kOffKept);
  uint32_t* total = reinterpret_cast<uint32_t*>(scratch + kOffTotal);
  const Pass* passes = sizeof(T) == 4 ? kPasses32 : kPasses64;
  const int npass = sizeof(T) == 4 ? 3 : 6;
  const Grid g = wave_grid(n, (uintptr_t)keys);

  // k == n: threshold key 0 with quota 0 drops nothing; k == 0: a threshold
  // above every key drops everything; neither needs the digit passes
  const bool select = k > 0 && k < n;
  const uint64_t prefix0 = k == 0 ? ~(uint64_t)0 : 0;
  hipLaunchKernelGGL(k_init, dim3(1), dim3(kBlock), 0, s, st, hist, prefix0, (uint32_t)(select ? n - k - 1 : 0));
  SA_HIP_CHECK(hipGetLastError());
  for (int p = 0; select && p < npass; p++) {
    hipLaunchKernelGGL(k_hist<T>, dim3(g.grid), dim3(kBlock), 0, s, keys, n, g.len, g.vec, (const State*)st, hist,
                       passes[p].shift, 1 << passes[p].bits);
    SA_HIP_CHECK(hipGetLastError());
    if (passes[p].bits == 11)
      hipLaunchKernelGGL(k_scan<kMaxBins / kBlock>, dim3(1), dim3(kBlock), 0, s, hist, passes[p].shift,
                         p == npass - 1, st);
    else
      hipLaunchKernelGGL(k_scan<1024 / kBlock>, dim3(1), dim3(kBlock), 0, s, hist, passes[p].shift,
                         p == npass - 1, st);
    SA_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_count<T>, dim3(g.grid), dim3(kBlock), 0, s, keys, n, g.len, g.vec, (const State*)st, ties,
                     kept);
  SA_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_offsets, dim3(1), dim3(kBlock), 0, s, ties, kept, g.nwaves, (const State*)st, total);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

template <class KT, class XT>
static int launch_fill(const KT* keys, const XT* x, uint64_t n, uint64_t k, const char* scratch, int32_t* index_out,
                       XT* data_out, uint32_t* flag, hipStream_t s) {
  const Grid g = wave_grid(n, (uintptr_t)keys | (uintptr_t)x);
  hipLaunchKernelGGL((k_fill<KT, XT>), dim3(g.grid), dim3(kBlock), 0, s, keys, x, n, g.len, g.vec,
                     reinterpret_cast<const State*>(scratch), reinterpret_cast<const uint32_t*>(scratch + kOffTies),
                     reinterpret_cast<const uint32_t*>(scratch + kOffKept),
                     reinterpret_cast<const uint32_t*>(scratch + kOffTotal), index_out, data_out, (uint32_t)k, flag);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

}  // namespace topk
}  // namespace sa

using namespace sa::topk;

extern "C" int sa_topk_scratch_bytes(uint64_t n, int key_type) {
  const int rc = check_type_n(key_type, n, "sa_topk_scratch_bytes");
  return rc == SA_OK ? (int)kScratchBytes : rc;
}

extern "C" int sa_topk_select(const void* keys, int key_type, uint64_t n, uint64_t k, void* scratch, void* stream) {
  int rc = check_type_n(key_type, n, "sa_topk_select");
  if (rc == SA_OK) rc = check_k(k, n, "sa_topk_select");
  if (rc != SA_OK) return rc;
  if (n == 0) return SA_OK;
  if (!keys || !scratch || misaligned(keys, elem_size(key_type)) || misaligned(scratch, 8)) {
    sa_set_error("sa_topk_select: bad arguments (keys and scratch are required; element-aligned keys, 8-byte "
                 "aligned scratch)");
    return SA_ERR_ARG;
  }
  return dispatch_float(key_type, [&](auto t) {
    typedef decltype(t) T;
    return launch_select((const T*)keys, n, k, (char*)scratch, (hipStream_t)stream);
  });
}

extern "C" int sa_topk_fill(const void* keys, int key_type, const void* x, int x_type, uint64_t n, uint64_t k,
                            const void* scratch, void* index_out, void* data_out, void* flag, void* stream) {
  int rc = check_float(key_type, "sa_topk_fill", "key_type");
  if (rc == SA_OK) rc = check_float(x_type, "sa_topk_fill", "x_type");
  if (rc == SA_OK) rc = check_n(n, 31, "sa_topk_fill", " (the flat index is int32)");
  if (rc == SA_OK) rc = check_k(k, n, "sa_topk_fill");
  if (rc != SA_OK) return rc;
  if (n == 0) return SA_OK;
  const uintptr_t ksz = elem_size(key_type), xsz = elem_size(x_type);
  if (!keys || !x || !scratch || !flag || (k && (!index_out || !data_out)) || misaligned(keys, ksz) ||
      misaligned(x, xsz) || misaligned(scratch, 8) || misaligned(flag, 4) || misaligned(index_out, 4) ||
      misaligned(data_out, xsz)) {
    sa_set_error("sa_topk_fill: bad arguments (keys, x, scratch, flag and, for k > 0, index_out and data_out are "
                 "required; element-aligned vectors, 8-byte aligned scratch)");
    return SA_ERR_ARG;
  }
  if (x == keys && x_type != key_type) {
    sa_set_error("sa_topk_fill: x is keys itself only with keys' element type");
    return SA_ERR_ARG;
  }
  const struct {
    const void* p;
    uint64_t bytes;
  } in[] = {{keys, n * ksz}, {x, n * xsz}, {scratch, kScratchBytes}, {flag, 8}, {data_out, k * xsz}};
  for (int i = 0; i < 5; i++) {
    if (overlap(index_out, k * 4, in[i].p, in[i].bytes) || (i < 4 && overlap(data_out, k * xsz, in[i].p, in[i].bytes))) {
      sa_set_error("sa_topk_fill: index_out and data_out may alias nothing");
      return SA_ERR_ARG;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  return dispatch_float(key_type, [&](auto kt) {
    typedef decltype(kt) KT;
    return dispatch_float(x_type, [&](auto xt) {
      typedef decltype(xt) XT;
      return launch_fill((const KT*)keys, (const XT*)x, n, k, (const char*)scratch, (int32_t*)index_out,
                         (XT*)data_out, (uint32_t*)flag, s);
    });
  });
}

static int check_random_keys(uint64_t n, const void* keys_out, const char* what) {
  const int rc = check_n(n, 31, what, " (the flat index is int32)");
  if (rc != SA_OK || n == 0) return rc;
  if (!keys_out || misaligned(keys_out, 8)) {
    sa_set_error("%s: keys_out is required and 8-byte aligned", what);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

extern "C" int sa_topk_random_keys(uint64_t seed, uint64_t n, void* keys_out, void* stream) {
  const int rc = check_random_keys(n, keys_out, "sa_topk_random_keys");
  if (rc != SA_OK || n == 0) return rc;
  uint64_t blocks = ((n + 1) / 2 + kBlock - 1) / kBlock;
  if (blocks > (uint64_t)kMaxBlocks * 4) blocks = (uint64_t)kMaxBlocks * 4;
  hipLaunchKernelGGL(k_random_keys, dim3((int)blocks), dim3(kBlock), 0, (hipStream_t)stream, seed, n,
                     (int)sa::aligned16(keys_out), (uint64_t*)keys_out);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_topk_random_keys_host(uint64_t seed, uint64_t n, void* keys_out_) {
  uint64_t* keys_out = (uint64_t*)keys_out_;
  const int rc = check_random_keys(n, keys_out, "sa_topk_random_keys_host");
  if (rc != SA_OK || n == 0) return rc;
  for (uint64_t b = 0; 2 * b < n; b++) {
    uint32_t c[4] = {(uint32_t)b, (uint32_t)(b >> 32), 0u, 0u};
    sa::philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    keys_out[2 * b] = key63(c[0], c[1]);
    if (2 * b + 1 < n) keys_out[2 * b + 1] = key63(c[2], c[3]);
  }
  return SA_OK;
}
