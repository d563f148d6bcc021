// sa_select.h — the radix SELECT on a magnitude key that sa_stc.hip and
// sa_topk.hip share: the key of an element, the select's state, the block's
// histogram in LDS and the three kernels that narrow (prefix, rank) one digit
// per pass.
//
// Included INSIDE the includer's namespace (sa::stc, sa::topk), after
// sa_compress.h and the includer's using-directives for sa::elems and
// sa::wave: every includer gets its own kernels under its own names, so a
// profile tells whose pass it sees and sa_stc's symbols and code are what they
// were before this header existed.  Nothing else includes it.

constexpr int kMaxBins = 2048;
// LDS copies of the histogram: lane l adds into copy l % 4, so lanes of one
// wave-instruction that share a digit (the first pass's digit is the
// exponent) serialise four times less often; the copies of a bin sit in four
// neighbouring banks and are read back as one 16-byte load.
constexpr int kCopies = 4;

// the select's state (scratch offset 0)
struct State {
  uint64_t prefix;  // the threshold key's digits found so far; at the end the threshold key
  uint32_t k;       // rank of the threshold element among the keys that match prefix
  uint32_t q;       // ties at the threshold that are masked (lowest indices first)
  double mu;        // value of T
  uint64_t pad[5];
};
static_assert(sizeof(State) == 64, "scratch layout");

template <class T>
struct Key;
template <>
struct Key<float> {
  typedef uint32_t type;
  static __device__ __forceinline__ uint32_t of(float x) { return __float_as_uint(x) & 0x7fffffffu; }
  static __device__ __forceinline__ float value(uint32_t k) { return __uint_as_float(k); }
};
template <>
struct Key<double> {
  typedef uint64_t type;
  static __device__ __forceinline__ uint64_t of(double x) {
    return (uint64_t)__double_as_longlong(x) & 0x7fffffffffffffffull;
  }
  static __device__ __forceinline__ double value(uint64_t k) { return __longlong_as_double((long long)k); }
};

// --- the block's histogram in LDS ---------------------------------------
__device__ __forceinline__ void hist_clear(uint32_t* h) {
  for (int i = threadIdx.x; i < kMaxBins * kCopies; i += kBlock) h[i] = 0;
  __syncthreads();
}

// One element per lane (`on`: the lane has one).  Called by the whole wave.
// The lanes that share the first active lane's digit are counted with one
// ballot and added once (a tensor of zeros, or a pass whose candidates all
// fall into one bin, would otherwise serialise 64 adds on one address); the
// others add 1 to their copy.
__device__ __forceinline__ void hist_add(uint32_t* h, uint32_t digit, bool on, int lane) {
  const uint64_t act = __ballot(on);
  if (act == 0) return;
  const int leader = __ffsll((unsigned long long)act) - 1;
  const uint32_t ld = (uint32_t)__shfl((int)digit, leader, 64);
  const bool same = on && digit == ld;
  const uint64_t sm = __ballot(same);
  if (lane == leader)
    atomicAdd(&h[ld * kCopies], (uint32_t)__popcll(sm));
  else if (on && !same)
    atomicAdd(&h[digit * kCopies + (lane & (kCopies - 1))], 1u);
}

// one integer atomic per non-empty bin: order-free, so deterministic
__device__ __forceinline__ void hist_flush(const uint32_t* h, uint32_t* g, int nbins) {
  __syncthreads();
  for (int b = threadIdx.x; b < nbins; b += kBlock) {
    const uint32_t c = (h[b * kCopies] + h[b * kCopies + 1]) + (h[b * kCopies + 2] + h[b * kCopies + 3]);
    if (c) atomicAdd(&g[b], c);
  }
}

// --- kernels --------------------------------------------------------------

// prefix / rank / quota for this call; the histogram starts at zero.
__global__ void __launch_bounds__(kBlock) k_init(State* st, uint32_t* hist, uint64_t prefix, uint32_t k) {
  for (int i = threadIdx.x; i < kMaxBins; i += kBlock) hist[i] = 0;
  if (threadIdx.x == 0) {
    st->prefix = prefix;
    st->k = k;
    st->q = 0;
    st->mu = 0.0;
  }
}

// histogram of digit (key >> shift) & (nbins - 1) over the keys whose higher
// digits equal the prefix found so far
template <class T>
__global__ void __launch_bounds__(kBlock) k_hist(const T* __restrict__ u, uint64_t n, uint64_t len, int vec,
                                                 const State* __restrict__ st, uint32_t* hist, int shift,
                                                 int nbins) {
  typedef typename Key<T>::type K;
  __shared__ __attribute__((aligned(16))) uint32_t h[kMaxBins * kCopies];
  hist_clear(h);
  const int hshift = shift + __builtin_ctz(nbins);  // < key bits: only the first digit reaches the top
  const K want = (K)st->prefix >> hshift;
  const Range w = wave_range(n, len);
  for (uint64_t t = w.lo; t < w.hi; t += 2 * kTile) {
    const uint64_t e0 = t + (uint64_t)w.lane * kEpl, e1 = e0 + kTile;
    const int c0 = lane_count(e0, w.hi), c1 = lane_count(e1, w.hi);
    const Elems<T> x0 = load_elems(u, e0, c0, vec);
    const Elems<T> x1 = load_elems(u, e1, c1, vec);
#pragma unroll
    for (int j = 0; j < kEpl; j++) {
      const K key = Key<T>::of(x0.v[j]);
      hist_add(h, (uint32_t)(key >> shift) & (uint32_t)(nbins - 1), j < c0 && (key >> hshift) == want, w.lane);
    }
#pragma unroll
    for (int j = 0; j < kEpl; j++) {
      const K key = Key<T>::of(x1.v[j]);
      hist_add(h, (uint32_t)(key >> shift) & (uint32_t)(nbins - 1), j < c1 && (key >> hshift) == want, w.lane);
    }
  }
  hist_flush(h, hist, nbins);
}

// One block: the bin that holds rank k; prefix |= bin << shift, k -= the
// count below it; the histogram is left zeroed for the next pass.
template <int PER>
__global__ void __launch_bounds__(kBlock) k_scan(uint32_t* hist, int shift, int last, State* st) {
  const uint32_t k = st->k;  // read by every thread before the barrier inside the scan
  uint32_t c[PER], s = 0;
#pragma unroll
  for (int j = 0; j < PER; j++) {
    c[j] = hist[threadIdx.x * PER + j];
    hist[threadIdx.x * PER + j] = 0;
    s += c[j];
  }
  uint32_t total;
  uint32_t run = block_scan_incl(s, &total) - s;
  if (k >= run && k < run + s) {  // exactly one thread: k < the count of the keys that match prefix
#pragma unroll
    for (int j = 0; j < PER; j++) {
      if (k >= run && k < run + c[j]) {
        st->prefix |= (uint64_t)(threadIdx.x * PER + j) << shift;
        st->k = k - run;
        if (last) st->q = k - run + 1;
      }
      run += c[j];
    }
  }
}

struct Pass {
  int shift, bits;
};
// float32: 31 key bits as 11/10/10; float64: 63 as 11/11/11/10/10/10
constexpr Pass kPasses32[] = {{20, 11}, {10, 10}, {0, 10}};
constexpr Pass kPasses64[] = {{52, 11}, {41, 11}, {30, 11}, {20, 10}, {10, 10}, {0, 10}};
