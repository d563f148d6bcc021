// sa_api.hip — the occupancy cache, the masking reserve and the masking
// entry points of libsfl_sa.so (see include/sfl_sa.h): sa_mask,
// sa_fused_clients, sa_fused_bipartite.  The server kernels are in
// sa_server.hip, the blocking host-array entries in sa_host_calls.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <unordered_map>

#include "../../include/sfl_sa.h"
#include "pcg128.h"
#include "sa_internal.h"
#include "sa_philox.h"

namespace sa {

// CUs' worth of the masking kernel's blocks left free for kernels on other
// streams (sa_set_masking_reserve); 0: the masking grid fills the GPU
static std::atomic<int> g_masking_reserve{0};

int masking_grid_cap(const void* kernel) {
  const int maxb = occupancy_blocks(kernel);
  const int reserve = g_masking_reserve.load(std::memory_order_relaxed);
  if (maxb <= 0 || reserve <= 0) return maxb;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
    sa_set_error("occupancy query failed");
    return -1;
  }
  const int keep = maxb - (maxb / cus) * reserve;
  return keep > maxb / 2 ? keep : maxb / 2;
}

int occupancy_blocks(const void* kernel) {
  static std::mutex mu;
  static std::unordered_map<const void*, int> cache;
  std::lock_guard<std::mutex> g(mu);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    sa_set_error("hipGetDevice failed");
    return -1;
  }
  const void* key = (const void*)((uintptr_t)kernel ^ ((uintptr_t)dev << 56));
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int per_cu = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlockThreads, 0) !=
          hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
    sa_set_error("occupancy query failed");
    return -1;
  }
  if (per_cu < 1) per_cu = 1;
  const int blocks = per_cu * cus;
  cache[key] = blocks;
  return blocks;
}

int check_type(int t, const char* what) {
  if (t != SA_F32 && t != SA_F64 && t != SA_I64) {
    sa_set_error("%s: unknown element type %d", what, t);
    return SA_ERR_ARG;
  }
  return SA_OK;
}

static bool valid_sign(int sign) { return sign == 1 || sign == -1; }

// One launch's kernel arguments, built in the order: base image, client
// slots, streams, outputs.
struct LaunchArgs {
  KArgs a;

  // zeroed, with n, fxp_bits and the scales 2^fxp_bits (0: the masks-only launches, scale 1)
  LaunchArgs(uint64_t n, int fxp_bits) {
    memset(&a, 0, sizeof(a));
    a.n = n;
    a.fxp_bits = fxp_bits;
    a.scale_d = (double)((uint64_t)1 << fxp_bits);
    a.scale_f = (float)a.scale_d;
  }

  void client(int c, const void* x, const void* wvec, uint64_t* masked_out, double w) {
    a.c[c].x = x;
    a.c[c].wvec = wvec;
    a.c[c].masked_out = masked_out;
    a.c[c].w = w;
    a.c[c].ws[0] = a.c[c].ws[1] = (float)w * a.scale_f;  // IEEE single multiply, as __fmul_rn on the device
  }

  // Stream `slot` (still zero) of generator g: client u adds it with `sign`;
  // for a pair stream client v subtracts what u adds.  false: sign is not
  // +1 / -1.  The kernel draws t = raw (sign +1) or t = ~raw (sign -1) once,
  // u takes +t and v takes -t; the mask is m = raw + K (K = kMaskOffset), so
  // what is left goes into the biases:
  //   sign +1: u adds m = t + K;           v subtracts it: -t - K
  //   sign -1: u gets -m = t + (1 - K);    v gets +m = -t + (K - 1)
  bool stream(int slot, const sa_pcg64& g, int sign, int u, int v = -1) {
    if (!valid_sign(sign)) return false;
    StreamSeed& s = a.seed[slot];
    s.s_lo = g.state.lo;
    s.s_hi = g.state.hi;
    s.inc_lo = g.inc.lo;
    s.inc_hi = g.inc.hi;
    if (sign < 0) a.sub_mask |= 1u << slot;
    const uint64_t fold = sign > 0 ? kMaskOffset : 1 - kMaskOffset;
    a.c[u].bias += fold;
    if (v >= 0) a.c[v].bias -= fold;
    return true;
  }

  // sum_mode: 0 none, 1 store, 2 accumulate (0 where there is no sum_out)
  const KArgs& outputs(uint64_t* sum_out, int sum_mode, uint64_t* digests, uint32_t* flags) {
    a.sum_out = sum_out;
    a.sum_mode = sum_out ? sum_mode : 0;
    a.digests = digests;
    a.do_digest = digests ? 1 : 0;
    a.flags = flags;
    return a;
  }
};

}  // namespace sa

using namespace sa;

extern "C" int sa_mask(const void* x, int x_type, int compute_type, uint64_t n, double weight,
                       const void* weight_vec, int fxp_bits, const sa_mask_stream* streams,
                       int n_streams, uint64_t* out, uint64_t* sum_accum, uint64_t* digest,
                       uint32_t* flags, void* stream) {
  return sa_mask_impl(x, x_type, compute_type, n, weight, weight_vec, fxp_bits, streams, n_streams, out,
                      sum_accum, digest, flags, stream, nullptr);
}

int sa_mask_impl(const void* x, int x_type, int compute_type, uint64_t n, double weight, const void* weight_vec,
                 int fxp_bits, const sa_mask_stream* streams, int n_streams, uint64_t* out, uint64_t* sum_accum,
                 uint64_t* digest, uint32_t* flags, void* stream, const sa_dp* dp) {
  if (check_type(x_type, "sa_mask x_type") || check_type(compute_type, "sa_mask compute_type"))
    return SA_ERR_ARG;
  if (n == 0 && n_streams >= 0 && fxp_bits >= 0 && fxp_bits <= 62) return SA_OK;  // nothing to touch
  if (!out || n_streams < 0 || (n_streams > 0 && !streams) || fxp_bits < 0 || fxp_bits > 62) {
    sa_set_error("sa_mask: bad arguments (out=%p n_streams=%d fxp_bits=%d)", (void*)out,
                 n_streams, fxp_bits);
    return SA_ERR_ARG;
  }
  if (!aligned16(x) || !aligned16(out) || !aligned16(weight_vec) || !aligned16(sum_accum)) {
    sa_set_error("sa_mask: device buffers must be 16-byte aligned");
    return SA_ERR_ARG;
  }
  // fp32 has kernels for up to 16 streams per pass, the other types 8
  const int per_pass = (x_type == SA_F32 && compute_type == SA_F32) ? kMaskPass : kMaskPass / 2;
  const int passes = n_streams == 0 ? 1 : (n_streams + per_pass - 1) / per_pass;
  for (int p = 0; p < passes; p++) {
    const int j0 = p * per_pass;
    const int cnt = n_streams - j0 < per_pass ? n_streams - j0 : per_pass;
    const bool last = p == passes - 1;
    LaunchArgs b(n, fxp_bits);
    b.a.continue_mode = (p > 0 || x == nullptr) ? 1 : 0;
    b.client(0, x, weight_vec, out, weight);
    for (int j = 0; j < cnt; j++)
      if (!b.stream(j, streams[j0 + j].gen, streams[j0 + j].sign, 0)) {
        sa_set_error("sa_mask: stream %d has sign %d (want +1/-1)", j0 + j, streams[j0 + j].sign);
        return SA_ERR_ARG;
      }
    if (dp) {
      b.a.dp_on = 1;
      b.a.dp_clip = dp->l2_norm_clip;
      b.a.dp_sigma = dp->noise_std;
      b.a.dp_updates = dp->num_updates;
      b.a.dp_inv = exact_recip_pow2(dp->num_updates);
      b.a.dp_sumsq = dp->sumsq;
      b.a.dp_sumsq_layer = dp->sumsq_layer;
      b.a.dp_key = dp->key;
      b.a.dp_block0 = dp->counter0 / 4;
    }
    const KArgs& a = b.outputs(last ? sum_accum : nullptr, 2, last ? digest : nullptr, flags);
    const int ct = compute_type;
    // the lean single-client kernel unless a general path is needed
    // (continue mode, per-element weights, DP): float32 kernels only
    LaunchFn fn = (!a.continue_mode && !weight_vec && !dp) ? find_clients_kernel(x_type, ct, 1, cnt, kLean1)
                                                           : nullptr;
    if (!fn) fn = find_clients_kernel(x_type, ct, 1, cnt);
    if (!fn) {
      sa_set_error("sa_mask: no kernel for x_type=%d compute_type=%d streams=%d", x_type, ct, cnt);
      return SA_ERR_UNSUPPORTED;
    }
    const int rc = fn(a, stream);
    if (rc) return rc;
  }
  return SA_OK;
}

// One masks-only launch: sum_out += sum over the cnt streams of +-(raw + K)
// mod 2^64 (the kCrossOnly kernel: no input vector, nothing quantized; its
// one client slot stays zero, the input is never read).
static int launch_cross_group(const sa_mask_stream* ms, int cnt, uint64_t n, uint64_t* sum_out, uint32_t* flags,
                              void* stream) {
  LaunchArgs b(n, 0);
  for (int j = 0; j < cnt; j++)
    if (!b.stream(j, ms[j].gen, ms[j].sign, 0)) {  // sa_fused_clients checked every sign before its first launch
      sa_set_error("masks-only launch: stream sign %d", ms[j].sign);
      return SA_ERR_ARG;
    }
  const LaunchFn fn = find_clients_kernel(SA_F32, SA_F32, 1, cnt, kLean1 | kSumOnly | kCrossOnly);
  if (!fn) {
    sa_set_error("masks-only launch: no kernel for %d streams", cnt);
    return SA_ERR_UNSUPPORTED;
  }
  return fn(b.outputs(sum_out, 2, nullptr, flags), stream);
}

// the masks-only launch sizes for `count` one-sided streams: the largest
// instantiated count (kCrossCounts) that fits the remaining streams
static int cross_launch_size(int remaining) {
  for (int c : kCrossCounts)
    if (c <= remaining) return c;
  return 1;
}

// every masks-only kernel the schedule of `count` streams needs exists
// (checked before anything is launched: see sa_fused_clients)
static bool cross_plan_instantiated(int count) {
  for (int j = 0; j < count; j += cross_launch_size(count - j))
    if (!find_clients_kernel(SA_F32, SA_F32, 1, cross_launch_size(count - j), kLean1 | kSumOnly | kCrossOnly))
      return false;
  return true;
}

// sum_out += the masks of `count` one-sided streams, in launches of the
// largest instantiated count (kCrossCounts) that fits the remaining streams.
static int launch_cross(const sa_mask_stream* ms, int count, uint64_t n, uint64_t* sum_out, uint32_t* flags,
                        void* stream) {
  for (int j = 0; j < count;) {
    const int cnt = cross_launch_size(count - j);
    const int rc = launch_cross_group(ms + j, cnt, n, sum_out, flags, stream);
    if (rc) return rc;
    j += cnt;
  }
  return SA_OK;
}

extern "C" int sa_fused_clients(const sa_local_client* clients, int n_clients, int x_type,
                                uint64_t n, int fxp_bits, const sa_pcg64* pair_gens,
                                const int8_t* pair_sign, const sa_mask_stream* cross,
                                int n_cross, uint64_t* sum_out, int accumulate,
                                uint64_t* digests, uint32_t* flags, void* stream) {
  if (check_type(x_type, "sa_fused_clients x_type")) return SA_ERR_ARG;
  const int L = n_clients;
  const int PI = L * (L - 1) / 2;
  if (n == 0 && L >= 1 && n_cross >= 0 && fxp_bits >= 0 && fxp_bits <= 62) return SA_OK;  // empty vectors
  if (!clients || L < 1 || n_cross < 0 || !sum_out || fxp_bits < 0 ||
      fxp_bits > 62 || (PI > 0 && (!pair_gens || !pair_sign)) || (n_cross > 0 && !cross)) {
    sa_set_error("sa_fused_clients: bad arguments (n_clients=%d n_cross=%d)", L, n_cross);
    return SA_ERR_ARG;
  }
  if (L > kMaxLocal) {  // valid, but one launch holds at most kMaxLocal clients' accumulators
    sa_set_error("sa_fused_clients: %d co-located clients exceed the %d per launch", L, kMaxLocal);
    return SA_ERR_UNSUPPORTED;
  }
  // anything but the sum wanted: per-client digests or wire images
  bool any_out = digests != nullptr;
  for (int c = 0; c < L; c++) any_out = any_out || clients[c].masked_out != nullptr;
  if (PI + L * n_cross > kMaxStreams) {
    // More streams than one launch holds (config 5 at 8 GPUs: 4 local clients,
    // 6 internal pairs + 4 x 28 cross streams).  With only the sum wanted, a
    // multi-launch schedule that still draws every internal pair ONCE: a
    // fused sum-only launch with the pairs and the first X1 cross streams of
    // every client, then masks-only launches of the remaining cross streams
    // adding into the sum (their per-client split does not matter there).
    int X1 = -1;
    if (!any_out && x_type == SA_F32)
      for (int x = n_cross - 1; x >= 0 && X1 < 0; x--)
        if (PI + L * x <= kMaxStreams && find_clients_kernel(x_type, x_type, L, x, (L == 1 ? kLean1 : 0) | kSumOnly))
          X1 = x;
    if (X1 < 0) {  // digests / wire images wanted, or no first launch: the caller masks client by client
      sa_set_error("sa_fused_clients: %d streams exceed the %d per launch", PI + L * n_cross, kMaxStreams);
      return SA_ERR_UNSUPPORTED;
    }
    for (int j = 0; j < L * n_cross; j++)
      if (!valid_sign(cross[j].sign)) {
        sa_set_error("sa_fused_clients: cross stream %d sign %d", j, cross[j].sign);
        return SA_ERR_ARG;
      }
    sa_mask_stream first[kMaxStreams], rest[kMaxLocal * (kMaxStreams + 1)];
    if (L * (n_cross - X1) > (int)(sizeof(rest) / sizeof(rest[0]))) {
      sa_set_error("sa_fused_clients: %d cross streams per client exceed the multi-launch schedule", n_cross);
      return SA_ERR_UNSUPPORTED;
    }
    int nr = 0;
    for (int c = 0; c < L; c++)
      for (int j = 0; j < n_cross; j++) {
        if (j < X1)
          first[c * X1 + j] = cross[c * n_cross + j];
        else
          rest[nr++] = cross[c * n_cross + j];
      }
    // all-or-nothing: SA_ERR_UNSUPPORTED tells the caller nothing ran (it
    // then masks client by client into the same sum_out), so every kernel
    // of the schedule is looked up BEFORE the first launch, and a failure
    // after it is reported as SA_ERR_HIP (sum_out partly written)
    if (!cross_plan_instantiated(nr)) {
      sa_set_error("sa_fused_clients: no masks-only kernel for part of %d cross streams", nr);
      return SA_ERR_UNSUPPORTED;
    }
    const int rc = sa_fused_clients(clients, L, x_type, n, fxp_bits, pair_gens, pair_sign, first, X1, sum_out,
                                    accumulate, nullptr, flags, stream);
    if (rc) return rc;
    const int rc2 = launch_cross(rest, nr, n, sum_out, flags, stream);
    if (rc2 == SA_ERR_UNSUPPORTED) {
      sa_set_error("sa_fused_clients: masks-only launch failed after the first launch (sum_out partly written)");
      return SA_ERR_HIP;
    }
    return rc2;
  }
  if (!aligned16(sum_out)) {
    sa_set_error("sa_fused_clients: sum_out must be 16-byte aligned");
    return SA_ERR_ARG;
  }
  LaunchArgs b(n, fxp_bits);
  for (int c = 0; c < L; c++) {
    if (!clients[c].x || !aligned16(clients[c].x) || ((uintptr_t)clients[c].masked_out & 7)) {
      sa_set_error("sa_fused_clients: client %d x null or buffers not 16-byte aligned", c);
      return SA_ERR_ARG;
    }
    b.client(c, clients[c].x, nullptr, clients[c].masked_out, clients[c].weight);
  }
  int p = 0;
  for (int u = 0; u < L; u++)
    for (int v = u + 1; v < L; v++, p++)
      if (!b.stream(p, pair_gens[p], pair_sign[p], u, v)) {
        sa_set_error("sa_fused_clients: pair %d sign %d", p, pair_sign[p]);
        return SA_ERR_ARG;
      }
  for (int c = 0; c < L; c++)
    for (int j = 0; j < n_cross; j++) {
      const sa_mask_stream& ms = cross[c * n_cross + j];
      if (!b.stream(PI + c * n_cross + j, ms.gen, ms.sign, c)) {
        sa_set_error("sa_fused_clients: cross stream (%d,%d) sign %d", c, j, ms.sign);
        return SA_ERR_ARG;
      }
    }
  // one client: the lean kernel (a fused launch never uses the general
  // paths); only the sum wanted: the sum-only instantiation where there is one
  const int lean = L == 1 ? kLean1 : 0;
  LaunchFn fn = any_out ? nullptr : find_clients_kernel(x_type, x_type, L, n_cross, lean | kSumOnly);
  if (!fn && lean) fn = find_clients_kernel(x_type, x_type, 1, n_cross, kLean1);
  if (!fn) fn = find_clients_kernel(x_type, x_type, L, n_cross);
  if (!fn) {
    sa_set_error("sa_fused_clients: no kernel for x_type=%d clients=%d cross=%d", x_type, L,
                 n_cross);
    return SA_ERR_UNSUPPORTED;
  }
  return fn(b.outputs(sum_out, accumulate ? 2 : 1, digests, flags), stream);
}

extern "C" int sa_fused_bipartite(const sa_local_client* clients, int x_type, uint64_t n, int fxp_bits,
                                  const sa_pcg64* pair_gens, const int8_t* pair_sign, uint64_t* sum_out,
                                  int accumulate, uint32_t* flags, void* stream) {
  constexpr int L = kBipartiteClients, H = L / 2, PB = H * (L - H);
  if (check_type(x_type, "sa_fused_bipartite x_type")) return SA_ERR_ARG;
  if (n == 0 && fxp_bits >= 0 && fxp_bits <= 62) return SA_OK;  // empty vectors
  if (!clients || !pair_gens || !pair_sign || !sum_out || fxp_bits < 0 || fxp_bits > 62) {
    sa_set_error("sa_fused_bipartite: bad arguments");
    return SA_ERR_ARG;
  }
  if (!aligned16(sum_out)) {
    sa_set_error("sa_fused_bipartite: sum_out must be 16-byte aligned");
    return SA_ERR_ARG;
  }
  LaunchArgs b(n, fxp_bits);
  for (int c = 0; c < L; c++) {
    if (clients[c].x || clients[c].masked_out) {
      sa_set_error("sa_fused_bipartite: client %d: masks only (x and masked_out must be NULL)", c);
      return SA_ERR_ARG;
    }
    b.client(c, nullptr, nullptr, nullptr, clients[c].weight);
  }
  for (int p = 0; p < PB; p++)  // pair p = (p / (L - H), H + p % (L - H)), the kernel's Pairs<L, kBipartite>
    if (!b.stream(p, pair_gens[p], pair_sign[p], p / (L - H), H + p % (L - H))) {
      sa_set_error("sa_fused_bipartite: pair %d sign %d", p, pair_sign[p]);
      return SA_ERR_ARG;
    }
  LaunchFn fn = find_clients_kernel(x_type, x_type, L, 0, kBipartite);
  if (!fn) {
    sa_set_error("sa_fused_bipartite: no kernel for x_type=%d", x_type);
    return SA_ERR_UNSUPPORTED;
  }
  return fn(b.outputs(sum_out, accumulate ? 2 : 1, nullptr, flags), stream);
}

extern "C" int sa_set_masking_reserve(int cus) {
  if (cus < 0 || cus > 128) {
    sa_set_error("sa_set_masking_reserve: %d CUs (0..128)", cus);
    return SA_ERR_ARG;
  }
  g_masking_reserve.store(cus, std::memory_order_relaxed);
  return SA_OK;
}
