// sa_hist.hip — FeatureHistogram on the device: the node histograms of the
// reference's homo_boost (sfl/ml/boost/homo_boost/tree_core/
// feature_histogram.py:99-287; sfl_amd/ml/boost/feature_histogram.py has the
// definition and the host form).  Three passes:
//
//   codes   x (rows x F, row-major) -> uint8 codes, code = the number of the
//           feature's split points <= x; once per data set
//   build   codes, node_of_row, grad, hess -> the int64 image
//           (G, H, N)[slot][feature][code]: the hot path, once per layer
//   finish  the image -> float64 triples, cumulative over the codes
//
// Gradients are summed as integers (q = rint(v * 2^k), k chosen on the host so
// that no sum overflows), with integer atomics in LDS and in global memory:
// the image does not depend on the order of the adds, so the same input gives
// the same bits on every run and the bits of the numpy form.  No float
// atomics anywhere.
//
// build: grid = row tiles x feature groups.  A block of 256 threads keeps, in
// LDS, the accumulators of its feature group (fg features, a multiple of 4)
// for the launch's slots and all codes 0 .. Bmax; the code nb_f ("beyond")
// is a bin like any other and carries what use_missing needs.  A lane owns a
// row: it reads node_of_row, grad and hess once, forms q_grad and q_hess once,
// and spends them on the group's fg features, one dword of codes for four of
// them, three LDS integer atomics a feature.  At the end of its rows the block
// adds its non-zero entries into the image with global integer atomics.
// hist_geometry picks fg and the slots per launch from Bmax and the LDS
// budget; a batch with more slots runs as several launches over slot ranges.
#include <hip/hip_runtime.h>

#include "sa_compress.h"

namespace sa {
namespace hist {

using namespace sa::entry;
using namespace sa::wave;

constexpr int kMaxBins = SA_HIST_MAX_BINS;
constexpr int kTable = 256;     // entries of a feature's split-point table in LDS (255 + one pad)
constexpr int kCodeGroup = 8;   // features per block of the codes pass
constexpr int kMaxGroup = 16;   // features per block of the build pass, at most (four dwords of codes)
constexpr int kEntryBytes = 20;  // one (G, H, N) accumulator: 8 + 8 + 4
// LDS of a build block.  gfx950 has 160 KiB per CU; 64 KiB keeps two blocks
// resident with room to spare and needs no opt-in above the 64 KiB a launch
// may ask for by default.
constexpr int kLdsBudget = 65536;
constexpr int kMaxTiles = 1024;  // blocks of a build launch over all groups, about (2 resident per CU on 256 CUs) x 2

// --- geometry (host) ----------------------------------------------------------

struct Geometry {
  int fg;        // features per block (4, 8 or 16)
  int slots;     // slots per launch
  int launches;  // ceil(n_nodes / slots)
  int lds;       // bytes of LDS of a block of the first launch
};

// The feature-group width and the slots per launch for histograms of bmax
// split points at most, n_nodes slots and F features: of fg in {16, 8, 4} the
// one with the fewest bytes read per row, launches x groups x (fg code bytes +
// node_of_row + grad + hess), the wider on a tie.  bmax in 0..255, n_nodes
// and F >= 1.
inline Geometry hist_geometry(int bmax, int n_nodes, uint64_t F) {
  const int per_sf = (bmax + 1) * kEntryBytes;
  Geometry best = {0, 0, 0, 0};
  uint64_t best_cost = ~0ull;
  for (int fg = kMaxGroup; fg >= 4; fg >>= 1) {
    if (fg > 4 && (uint64_t)fg >= F + 4) continue;  // wider than the features rounded up to a dword
    int slots = kLdsBudget / (fg * per_sf);
    if (slots == 0) continue;
    if (slots > n_nodes) slots = n_nodes;
    const int launches = (n_nodes + slots - 1) / slots;
    const uint64_t cost = (uint64_t)launches * ((F + fg - 1) / fg) * (uint64_t)(fg + 12);
    if (cost < best_cost) best_cost = cost, best = {fg, slots, launches, slots * fg * per_sf};
  }
  return best;  // fg = 4 always fits: 4 x 256 x 20 bytes a slot, three slots in the budget
}

// --- codes ------------------------------------------------------------------------

// the number of the p - 1 table entries <= v, a branch-free binary search of
// log2(p) <= 8 probes; the pad entries are NaN and never count; a NaN v counts none
__device__ __forceinline__ uint32_t code_of(const double* tab, int p, double v) {
  uint32_t pos = 0;
  for (int step = p >> 1; step > 0; step >>= 1) pos += tab[pos + step - 1] <= v ? step : 0;
  return pos;
}

// A block: kCodeGroup features (blockIdx.y) of its rows; a thread a row.
// splits: the features' split points back to back in float64, feature f's at
// [offs[f], offs[f + 1]); p: the power of two above the largest count.
template <class T>
__global__ void __launch_bounds__(kBlock) k_codes(const T* __restrict__ x, uint64_t rows, uint64_t F,
                                                  const double* __restrict__ splits, const int32_t* __restrict__ offs,
                                                  int p, int vec, uint8_t* __restrict__ codes) {
  __shared__ double tab[kCodeGroup * kTable];
  __shared__ int nb[kCodeGroup];
  const uint64_t f0 = (uint64_t)blockIdx.y * kCodeGroup;
  const int nf = F - f0 < (uint64_t)kCodeGroup ? (int)(F - f0) : kCodeGroup;
  for (int i = threadIdx.x; i < nf * p; i += kBlock) {
    const int j = i / p, e = i - j * p;
    const int lo = offs[f0 + j], cnt = offs[f0 + j + 1] - lo;
    tab[j * kTable + e] = e < cnt ? splits[lo + e] : __builtin_nan("");
    if (e == 0) nb[j] = cnt;
  }
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < rows; r += stride) {
    const T* xr = x + r * F + f0;
    uint8_t* cr = codes + r * F + f0;
    uint32_t c[kCodeGroup];
#pragma unroll
    for (int j = 0; j < kCodeGroup; j++) {
      c[j] = 0;
      if (j < nf) {
        const double v = (double)xr[j];
        c[j] = v != v ? (uint32_t)nb[j] : code_of(tab + j * kTable, p, v);
      }
    }
    if (vec) {  // F a multiple of 4 and dword-aligned codes: whole dwords, nf a multiple of 4
#pragma unroll
      for (int d = 0; d < kCodeGroup / 4; d++)
        if (4 * d < nf)
          *reinterpret_cast<uint32_t*>(cr + 4 * d) = c[4 * d] | c[4 * d + 1] << 8 | c[4 * d + 2] << 16 | c[4 * d + 3] << 24;
    } else {
#pragma unroll
      for (int j = 0; j < kCodeGroup; j++)
        if (j < nf) cr[j] = (uint8_t)c[j];
    }
  }
}

// --- build ------------------------------------------------------------------------

struct Image {
  unsigned long long* g;
  unsigned long long* h;
  uint32_t* n;
};
// the image in scratch: G and H of every (slot, feature, code), then N
inline Image image_of(void* scratch, uint64_t entries) {
  Image im;
  im.g = (unsigned long long*)scratch;
  im.h = im.g + entries;
  im.n = (uint32_t*)(im.h + entries);
  return im;
}

__global__ void __launch_bounds__(kBlock) k_clear(uint32_t* p, uint64_t words) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < words) p[i] = 0;
}

// q = int64(rint(v * 2^k)): exact scaling, one rounding (np.rint: half to even)
template <class T>
__device__ __forceinline__ long long quantize(T v, int k) {
  return (long long)rint(ldexp((double)v, k));
}

// The four codes of features f .. f + 3 of a row: one dword where the rows
// are dword-aligned (vec), bytes otherwise; a feature beyond F gives 0xff,
// which no table holds.
__device__ __forceinline__ uint32_t load_codes4(const uint8_t* row, uint64_t f, uint64_t F, int vec) {
  if (vec) return *reinterpret_cast<const uint32_t*>(row + f);
  uint32_t w = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) w |= (f + j < F ? (uint32_t)row[f + j] : 0xffu) << (8 * j);
  return w;
}

// Rows [lo, hi) of block x, features [f0, f0 + fg) of block y, slots [slot0,
// slot0 + nslots).  LDS: G, H (64-bit) and N (32-bit) at [(slot * fg + feature)
// * ncodes + code].  A code above Bmax (another party's data) is never an index.
template <class T>
__global__ void __launch_bounds__(kBlock) k_build(const uint8_t* __restrict__ codes, uint64_t rows, uint64_t F,
                                                  uint64_t len, int vec, const int32_t* __restrict__ node,
                                                  const T* __restrict__ grad, const T* __restrict__ hess, int kg, int kh,
                                                  int slot0, int nslots, int fg, int ncodes, Image im) {
  extern __shared__ unsigned long long lds[];
  const int entries = nslots * fg * ncodes;
  unsigned long long* lg = lds;
  unsigned long long* lh = lds + entries;
  uint32_t* ln = reinterpret_cast<uint32_t*>(lds + 2 * entries);
  for (int i = threadIdx.x; i < entries; i += kBlock) lg[i] = 0, lh[i] = 0, ln[i] = 0;
  __syncthreads();
  const uint64_t f0 = (uint64_t)blockIdx.y * fg;
  const uint64_t lo = (uint64_t)blockIdx.x * len;
  const uint64_t hi = lo + len < rows ? lo + len : rows;
  const int nd = fg >> 2;
  for (uint64_t r = lo + threadIdx.x; r < hi; r += kBlock) {
    const uint32_t s = (uint32_t)(node[r] - slot0);
    if (s >= (uint32_t)nslots) continue;  // slot -1, or a slot of another launch
    const uint8_t* row = codes + r * F;
    uint32_t w[kMaxGroup / 4];
#pragma unroll
    for (int d = 0; d < kMaxGroup / 4; d++) w[d] = d < nd && f0 + 4 * d < F ? load_codes4(row, f0 + 4 * d, F, vec) : ~0u;
    const unsigned long long qg = (unsigned long long)quantize(grad[r], kg);
    const unsigned long long qh = (unsigned long long)quantize(hess[r], kh);
    const uint32_t base = s * (uint32_t)fg;
#pragma unroll
    for (int d = 0; d < kMaxGroup / 4; d++) {
      if (d < nd) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t c = (w[d] >> (8 * j)) & 0xffu;
          if (c < (uint32_t)ncodes && f0 + 4 * d + j < F) {
            const uint32_t at = (base + 4 * d + j) * (uint32_t)ncodes + c;
            atomicAdd(&lg[at], qg);
            atomicAdd(&lh[at], qh);
            atomicAdd(&ln[at], 1u);
          }
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < entries; i += kBlock) {
    const uint32_t cnt = ln[i];
    if (cnt) {  // the entry of a feature beyond F stays zero
      const int sf = i / ncodes, c = i - sf * ncodes;
      const int sl = sf / fg, fl = sf - sl * fg;
      const uint64_t at = ((uint64_t)(slot0 + sl) * F + f0 + fl) * ncodes + c;
      atomicAdd(&im.g[at], lg[i]);
      atomicAdd(&im.h[at], lh[i]);
      atomicAdd(&im.n[at], cnt);
    }
  }
}

// --- finish -----------------------------------------------------------------------

// inclusive scan over the wave's lanes, sa_compress.h's block scan for one
// wave and 64-bit values
__device__ __forceinline__ long long wave_scan_incl(long long v, int lane) {
  for (int off = 1; off < 64; off <<= 1) {
    const long long u = __shfl_up(v, off, 64);
    if (lane >= off) v += u;
  }
  return v;
}

// a[j], j in 0..3, by selects: a run-time index would put the array into scratch memory
__device__ __forceinline__ long long pick(const long long (&a)[4], int j) {
  return j == 0 ? a[0] : j == 1 ? a[1] : j == 2 ? a[2] : a[3];
}

__device__ __forceinline__ void store3(double* o, double g, double h, double n) { o[0] = g, o[1] = h, o[2] = n; }

// One wave a (slot, feature): lane l holds codes 4 l .. 4 l + 3.  out[slot][f]
// [b] = (G, H, N) over code <= b for b < nb_f; with use_missing, bucket nb_f =
// the totals less bucket nb_f - 1; everything else, and a feature with nb[f] <
// 0 (not valid), zero.  bout: buckets per feature in out.
__global__ void __launch_bounds__(kBlock) k_finish(Image im, uint64_t pairs, uint64_t F, int ncodes,
                                                   const int32_t* __restrict__ nb, int kg, int kh, int use_missing,
                                                   int bout, double* __restrict__ out) {
  const uint64_t pair = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (pair >= pairs) return;
  const int lane = threadIdx.x & 63;
  const int nbf = nb[pair % F];
  double* o = out + pair * (uint64_t)bout * 3;
  if (nbf < 0 || nbf >= ncodes) {  // not valid (nb_f <= Bmax always: never an index past the image)
    for (int b = lane; b < bout; b += 64) store3(o + 3 * b, 0.0, 0.0, 0.0);
    return;
  }
  long long g[4], h[4], n[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int c = 4 * lane + j;
    const uint64_t at = pair * ncodes + c;
    g[j] = c < ncodes ? (long long)im.g[at] : 0;
    h[j] = c < ncodes ? (long long)im.h[at] : 0;
    n[j] = c < ncodes ? (long long)im.n[at] : 0;
    if (j) g[j] += g[j - 1], h[j] += h[j - 1], n[j] += n[j - 1];
  }
  const long long bg = wave_scan_incl(g[3], lane) - g[3], bh = wave_scan_incl(h[3], lane) - h[3],
                  bn = wave_scan_incl(n[3], lane) - n[3];
  // the totals, and bucket nb_f - 1 (zero for nb_f == 0), for the missing bucket
  const long long tg = __shfl(bg + g[3], 63, 64), th = __shfl(bh + h[3], 63, 64), tn = __shfl(bn + n[3], 63, 64);
  long long lg = 0, lh = 0, lc = 0;
  if (nbf > 0) {
    const int src = (nbf - 1) >> 2, j = (nbf - 1) & 3;
    const long long cg = bg + pick(g, j), ch = bh + pick(h, j), cn = bn + pick(n, j);  // j is uniform over the wave
    lg = __shfl(cg, src, 64), lh = __shfl(ch, src, 64), lc = __shfl(cn, src, 64);
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int b = 4 * lane + j;
    if (b >= bout) continue;
    if (b < nbf)
      store3(o + 3 * b, ldexp((double)(bg + g[j]), -kg), ldexp((double)(bh + h[j]), -kh), (double)(bn + n[j]));
    else if (b == nbf && use_missing)
      store3(o + 3 * b, ldexp((double)(tg - lg), -kg), ldexp((double)(th - lh), -kh), (double)(tn - lc));
    else
      store3(o + 3 * b, 0.0, 0.0, 0.0);
  }
  // bout <= 256 = 4 x 64: every bucket has a lane
}

// --- checks -----------------------------------------------------------------------

// the shape of a batch: SA_OK and *entries = n_nodes F (bmax + 1), or an error set
static int check_shape(uint64_t n_nodes, uint64_t F, int bmax, const char* what, uint64_t* entries) {
  if (bmax < 0 || bmax > kMaxBins) {
    sa_set_error("%s: bmax must be in 0..%d", what, kMaxBins);
    return SA_ERR_ARG;
  }
  if (n_nodes >> 24 || F >> 16) {  // a grid's y dimension takes the feature groups
    sa_set_error("%s: n_nodes must be below 2^24 and n_features below 2^16", what);
    return SA_ERR_ARG;
  }
  *entries = n_nodes * F * (uint64_t)(bmax + 1);
  if (*entries * kEntryBytes + 4 > 0x7fffffffull) {
    sa_set_error("%s: scratch above 2^31 - 1 bytes", what);
    return SA_ERR_UNSUPPORTED;
  }
  return SA_OK;
}

static int check_rows(uint64_t rows, const char* what) {
  if (rows >> 31) {
    sa_set_error("%s: rows must be below 2^31 (the counts are 32-bit)", what);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

static int check_scale(int k, const char* name, const char* what) {
  if (k < -2100 || k > 2100) {  // beyond what ldexp of a float64 can use
    sa_set_error("%s: %s must be in -2100..2100", what, name);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

static uint64_t scratch_bytes_of(uint64_t entries) { return (entries * kEntryBytes + 7) / 8 * 8; }

}  // namespace hist
}  // namespace sa

using namespace sa::hist;

extern "C" int sa_hist_scratch_bytes(uint64_t n_nodes, uint64_t n_features, int bmax) {
  uint64_t entries;
  const int rc = check_shape(n_nodes, n_features, bmax, "sa_hist_scratch_bytes", &entries);
  return rc == SA_OK ? (int)scratch_bytes_of(entries) : rc;
}

extern "C" int sa_hist_geometry(int bmax, int n_nodes, uint64_t n_features, int* out4) {
  uint64_t entries;
  const int rc = check_shape(n_nodes < 0 ? ~0ull : (uint64_t)n_nodes, n_features, bmax, "sa_hist_geometry", &entries);
  if (rc != SA_OK) return rc;
  if (n_nodes < 1 || n_features < 1 || !out4) {
    sa_set_error("sa_hist_geometry: at least one node and one feature, and out4 is required");
    return SA_ERR_ARG;
  }
  const Geometry g = hist_geometry(bmax, n_nodes, n_features);
  out4[0] = g.fg, out4[1] = g.slots, out4[2] = g.launches, out4[3] = g.lds;
  return SA_OK;
}

extern "C" int sa_hist_codes(const void* x, int x_type, uint64_t rows, uint64_t n_features, const double* splits,
                             const int32_t* offsets, int bmax, uint8_t* codes_out, void* stream) {
  int rc = check_float(x_type, "sa_hist_codes");
  if (rc == SA_OK) rc = check_rows(rows, "sa_hist_codes");
  uint64_t entries;
  if (rc == SA_OK) rc = check_shape(1, n_features, bmax, "sa_hist_codes", &entries);
  if (rc != SA_OK) return rc;
  if (rows == 0 || n_features == 0) return SA_OK;
  if (!x || misaligned(x, elem_size(x_type)) || !offsets || misaligned(offsets, 4) || !codes_out ||
      (bmax && !splits) || misaligned(splits, 8)) {
    sa_set_error("sa_hist_codes: bad arguments (x, splits, offsets and codes_out are required; element-aligned x, "
                 "8-byte aligned splits, 4-byte aligned offsets)");
    return SA_ERR_ARG;
  }
  int p = 1;
  while (p <= bmax) p <<= 1;  // p - 1 >= bmax table entries
  uint64_t gx = (rows + kBlock - 1) / kBlock;
  const uint64_t gy = (n_features + kCodeGroup - 1) / kCodeGroup;
  if (gx > (uint64_t)kMaxBlocks) gx = kMaxBlocks;
  const int vec = (n_features & 3) == 0 && ((uintptr_t)codes_out & 3) == 0;
  hipStream_t st = (hipStream_t)stream;
  dispatch_float(x_type, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL(k_codes<T>, dim3((unsigned)gx, (unsigned)gy), dim3(kBlock), 0, st, (const T*)x, rows, n_features,
                       splits, offsets, p, vec, codes_out);
  });
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_hist_build(const uint8_t* codes, uint64_t rows, uint64_t n_features, int bmax,
                             const int32_t* node_of_row, int n_nodes, const void* grad, const void* hess, int g_type,
                             int k_grad, int k_hess, void* scratch, void* stream) {
  int rc = check_float(g_type, "sa_hist_build", "the gradients' type");
  if (rc == SA_OK) rc = check_rows(rows, "sa_hist_build");
  uint64_t entries;
  if (rc == SA_OK)
    rc = check_shape(n_nodes < 0 ? ~0ull : (uint64_t)n_nodes, n_features, bmax, "sa_hist_build", &entries);
  if (rc == SA_OK) rc = check_scale(k_grad, "k_grad", "sa_hist_build");
  if (rc == SA_OK) rc = check_scale(k_hess, "k_hess", "sa_hist_build");
  if (rc != SA_OK) return rc;
  if (entries == 0) return SA_OK;
  if (!scratch || misaligned(scratch, 8)) {
    sa_set_error("sa_hist_build: scratch is required and 8-byte aligned");
    return SA_ERR_ARG;
  }
  const uintptr_t esz = elem_size(g_type);
  if (rows && (!codes || !node_of_row || misaligned(node_of_row, 4) || !grad || !hess || misaligned(grad, esz) ||
               misaligned(hess, esz))) {
    sa_set_error("sa_hist_build: bad arguments (codes, node_of_row, grad and hess are required; 4-byte aligned "
                 "node_of_row, element-aligned grad and hess)");
    return SA_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const Image im = image_of(scratch, entries);
  const uint64_t words = scratch_bytes_of(entries) / 4;
  hipLaunchKernelGGL(k_clear, dim3((unsigned)((words + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, (uint32_t*)scratch,
                     words);
  if (rows) {
    const Geometry g = hist_geometry(bmax, n_nodes, n_features);
    const uint64_t groups = (n_features + g.fg - 1) / g.fg;
    uint64_t tiles = (rows + kBlock - 1) / kBlock;
    const uint64_t cap = (uint64_t)kMaxTiles / groups ? (uint64_t)kMaxTiles / groups : 1;
    if (tiles > cap) tiles = cap;
    uint64_t len = (rows + tiles - 1) / tiles;
    len = (len + kBlock - 1) / kBlock * kBlock;
    tiles = (rows + len - 1) / len;
    const int vec = (n_features & 3) == 0 && ((uintptr_t)codes & 3) == 0;
    for (int slot0 = 0; slot0 < n_nodes; slot0 += g.slots) {
      const int ns = n_nodes - slot0 < g.slots ? n_nodes - slot0 : g.slots;
      const size_t lds = (size_t)ns * g.fg * (bmax + 1) * kEntryBytes;
      dispatch_float(g_type, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_build<T>, dim3((unsigned)tiles, (unsigned)groups), dim3(kBlock), lds, st, codes, rows,
                           n_features, len, vec, node_of_row, (const T*)grad, (const T*)hess, k_grad, k_hess, slot0, ns,
                           g.fg, bmax + 1, im);
      });
    }
  }
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}

extern "C" int sa_hist_finish(const void* scratch, int n_nodes, uint64_t n_features, int bmax, const int32_t* n_bins,
                              int k_grad, int k_hess, int use_missing, double* out, void* stream) {
  uint64_t entries;
  int rc = check_shape(n_nodes < 0 ? ~0ull : (uint64_t)n_nodes, n_features, bmax, "sa_hist_finish", &entries);
  if (rc == SA_OK) rc = check_scale(k_grad, "k_grad", "sa_hist_finish");
  if (rc == SA_OK) rc = check_scale(k_hess, "k_hess", "sa_hist_finish");
  if (rc != SA_OK) return rc;
  const int bout = bmax + (use_missing ? 1 : 0);
  if (entries == 0 || bout == 0) return SA_OK;
  if (!scratch || misaligned(scratch, 8) || !n_bins || misaligned(n_bins, 4) || !out || misaligned(out, 8)) {
    sa_set_error("sa_hist_finish: bad arguments (scratch, n_bins and out are required; 8-byte aligned scratch and "
                 "out, 4-byte aligned n_bins)");
    return SA_ERR_ARG;
  }
  const uint64_t pairs = (uint64_t)n_nodes * n_features;  // below 2^31 / 20: the grid fits
  hipLaunchKernelGGL(k_finish, dim3((unsigned)((pairs + kWaves - 1) / kWaves)), dim3(kBlock), 0, (hipStream_t)stream,
                     image_of(const_cast<void*>(scratch), entries), pairs, n_features, bmax + 1, n_bins, k_grad, k_hess,
                     use_missing ? 1 : 0, bout, out);
  SA_HIP_CHECK(hipGetLastError());
  return SA_OK;
}
