// sa_flame_keys.h — what sa_flame.hip and sa_flame_wide.hip share: the packed
// layout of FlameAggregator's statistics, the integer keys by which the
// medians are ordered, Batcher's sorting network, and on the host the by-value
// argument structs and the entries' checks: the four entries of the two files
// differ in their client range and their launches only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sa_compress.h"

namespace sa {
namespace flame {

__host__ __device__ constexpr int gram_count(int c) { return c * (c + 1) / 2; }
__host__ __device__ constexpr int stat_count(int c) { return gram_count(c) + c; }
// the slot of G[i][i] in the packed upper triangle (row-major, j >= i)
__host__ __device__ constexpr int row_slot(int c, int i) { return i * c - i * (i - 1) / 2; }

// --- the order: integer keys --------------------------------------------------
template <class T>
struct Key;
template <>
struct Key<float> {
  typedef int32_t type;
  static constexpr int32_t kMag = 0x7fffffff;
};
template <>
struct Key<double> {
  typedef int64_t type;
  static constexpr int64_t kMag = 0x7fffffffffffffffll;
};

// the bit pattern as a signed integer whose order is the values' order with
// -0 < +0 (negative patterns have their magnitude bits flipped); its own inverse
template <class T>
__device__ __forceinline__ typename Key<T>::type to_key(T x) {
  typedef typename Key<T>::type K;
  K b;
  __builtin_memcpy(&b, &x, sizeof b);
  return b ^ ((b >> (8 * (int)sizeof(K) - 1)) & Key<T>::kMag);
}
template <class T>
__device__ __forceinline__ T from_key(typename Key<T>::type k) {
  typedef typename Key<T>::type K;
  const K b = k ^ ((k >> (8 * (int)sizeof(K) - 1)) & Key<T>::kMag);
  T x;
  __builtin_memcpy(&x, &b, sizeof x);
  return x;
}

// --- the sorting network --------------------------------------------------------
// Batcher's odd-even merge sort of C values as a list of compare-exchanges
// (lo, hi), lo < hi: the network of the next power of two without the
// exchanges that touch an index >= C (those values would be +infinity and
// never move).  63 exchanges at C = 16, 191 at 32, 543 at 64.
constexpr int kMaxExchanges = 576;
struct Net {
  int n;
  short lo[kMaxExchanges], hi[kMaxExchanges];
};
template <int C>
constexpr Net batcher() {
  Net net = {};
  for (int p = 1; p < C; p *= 2)
    for (int k = p; k >= 1; k /= 2)
      for (int j = k % p; j + k < C; j += 2 * k)
        for (int i = 0; i < k && i + j + k < C; i++)
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) net.lo[net.n] = i + j, net.hi[net.n] = i + j + k, net.n++;
  return net;
}

// --- the entries (host) -----------------------------------------------------------
// the kernels' by-value arguments: no device allocation holds the pointer table
template <int N>
struct ClientPtrs {
  const void* p[N];
};
template <int N>
struct ClientArgs {
  const void* p[N];
  double s[N], w[N];
};

// the client counts a file's entries take, and what a refusal says of them
struct ClientRange {
  int lo, hi;
  const char* note;
};
constexpr ClientRange kNarrow = {1, SA_FLAME_MAX_CLIENTS, "SA_FLAME_MAX_CLIENTS"};
constexpr ClientRange kWide = {SA_FLAME_MAX_CLIENTS + 1, SA_FLAME_WIDE_MAX_CLIENTS,
                               "SA_FLAME_WIDE_MAX_CLIENTS; 1..16: the sa_flame_* entries"};
static_assert(SA_FLAME_MAX_CLIENTS == 16, "kWide's note names the narrow entries' range");

// what every entry judges first: the element type, the size, the client count
inline int check_scalars(int x_type, uint64_t n, int n_clients, const ClientRange& r, const char* what) {
  const int rc = entry::check_float_n(x_type, n, 32, what);
  return rc != SA_OK ? rc : entry::check_clients(n_clients, r.lo, r.hi, what, r.note);
}

// A stats entry's checks.  n == 0 ends after stats (nothing else is looked
// at); else px gets the clients' pointers and *ptrs their addresses OR-ed.
inline int check_stats(const void* const* x, int n_clients, int x_type, uint64_t n, const void* median_out,
                       const void* scratch, const double* stats, const ClientRange& r, const char* what,
                       const void** px, uintptr_t* ptrs) {
  const int rc = check_scalars(x_type, n, n_clients, r, what);
  if (rc != SA_OK) return rc;
  const uintptr_t esz = entry::elem_size(x_type);
  if (!stats || entry::misaligned(stats, 8)) {
    sa_set_error("%s: bad arguments (stats is required, 8-byte aligned)", what);
    return SA_ERR_ARG;
  }
  if (n == 0) return SA_OK;
  if (!x || !median_out || !scratch || entry::misaligned(median_out, esz) || entry::misaligned(scratch, 8)) {
    sa_set_error("%s: bad arguments (x, median_out and scratch are required; element-aligned median_out, 8-byte "
                 "aligned scratch)", what);
    return SA_ERR_ARG;
  }
  return entry::take_table(x, n_clients, esz, px, what, "tensor", ptrs);
}

// A combine entry's checks and its walk of the clients: a dropped client (its
// weight is a NaN) is left out here, its pointer is not looked at and never
// reaches the kernel; the *kept others fill a from the front.  Dropping every
// client is refused, also for n == 0, which ends after that.
template <int N>
inline int check_combine(const void* const* x, const double* scale, const double* weight, int n_clients, int x_type,
                         uint64_t n, const void* median, const double* out, const ClientRange& r, const char* what,
                         ClientArgs<N>* a, int* kept, uintptr_t* ptrs) {
  int rc = check_scalars(x_type, n, n_clients, r, what);
  if (rc != SA_OK) return rc;
  const uintptr_t esz = entry::elem_size(x_type);
  if (!x || !scale || !weight) {
    sa_set_error("%s: bad arguments (x, scale and weight are required)", what);
    return SA_ERR_ARG;
  }
  for (int c = 0; c < n_clients; c++) {
    if (weight[c] != weight[c]) continue;
    if (n && (rc = entry::check_client(x[c], esz, what, c, "tensor")) != SA_OK) return rc;
    a->p[*kept] = x[c], a->s[*kept] = scale[c], a->w[*kept] = weight[c], *ptrs |= (uintptr_t)x[c];
    ++*kept;
  }
  if (*kept == 0) {
    sa_set_error("%s: every client is dropped (a NaN weight drops a client)", what);
    return SA_ERR_ARG;
  }
  if (n == 0) return SA_OK;
  if (!median || !out || entry::misaligned(median, esz) || entry::misaligned(out, 8)) {
    sa_set_error("%s: bad arguments (median and out are required; element-aligned median, 8-byte aligned out)", what);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

}  // namespace flame
}  // namespace sa
