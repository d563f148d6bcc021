// sa_host_calls.hip — the blocking small-call entries: host arrays in, host
// arrays out, one host-to-device and one device-to-host copy per call
// (sa_fused_clients_host_f32, sa_clients_host, sa_mask_host,
// sa_sum_decode_host).  Each reads as: layout (sa_host_layout.h), stage and
// upload, its device steps, finish.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/sfl_sa.h"
#include "sa_host_layout.h"
#include "sa_internal.h"

using namespace sa;

// An error after the first copy was enqueued drains the stream before
// returning, so the caller may reuse or free the scratch at once.
static int drain(hipStream_t s, int rc) {
  (void)hipStreamSynchronize(s);
  return rc;
}

static bool scratch_ok(const void* pinned, const void* dev) {
  return pinned && dev && aligned16(pinned) && aligned16(dev);
}

// every one of the n_vec host vectors is there, or "<entry>: <name>[c] is NULL"
static int check_vectors(const void* const* vecs, int n_vec, const char* entry, const char* name) {
  for (int c = 0; c < n_vec; c++)
    if (!vecs[c]) {
      sa_set_error("%s: %s[%d] is NULL", entry, name, c);
      return SA_ERR_ARG;
    }
  return SA_OK;
}

namespace {

// the steps the four entries share, over one call's layout and scratch
struct HostCall {
  const HostLayout l;
  char* const pin;
  char* const dev;
  const hipStream_t s;

  HostCall(const HostLayout& layout, void* pinned, void* device, void* stream)
      : l(layout), pin((char*)pinned), dev((char*)device), s((hipStream_t)stream) {}

  // on the device: the staged input c, the zeroed sum, the meta words, the result and the tail
  void* d_in(uint64_t c) const { return dev + c * l.in_stride; }
  uint64_t* d_zeroed() const { return (uint64_t*)(dev + l.zeroed); }
  uint64_t* d_meta() const { return (uint64_t*)(dev + l.meta); }
  void* d_result() const { return dev + l.result; }
  uint64_t* d_tail() const { return (uint64_t*)(dev + l.tail); }

  // stage the n_vec host vectors of `bytes` bytes each, then one
  // host-to-device copy of them and the zeroed words (a large sum is filled
  // on the device instead)
  int upload(const void* const* vecs, uint64_t n_vec, uint64_t bytes) const {
    for (uint64_t c = 0; c < n_vec; c++) memcpy(pin + c * l.in_stride, vecs[c], bytes);
    if (l.zero_by_copy) {
      memset(pin + l.zeroed, 0, l.result - l.zeroed);
      SA_HIP_CHECK_DRAIN(s, hipMemcpyAsync(dev, pin, l.result, hipMemcpyHostToDevice, s));
    } else {
      SA_HIP_CHECK_DRAIN(s, hipMemcpyAsync(dev, pin, l.zeroed, hipMemcpyHostToDevice, s));
      SA_HIP_CHECK_DRAIN(s, hipMemsetAsync(dev + l.zeroed, 0, l.result - l.zeroed, s));
    }
    return SA_OK;
  }

  // one device-to-host copy of the meta words and the n result elements,
  // synchronise, scatter: out[n], then the meta words in order -- the flag
  // word (its low half, little-endian) if `flags`, n_digests digests if `digests`
  int finish(uint64_t n, void* out, uint32_t* flags, uint64_t* digests, uint64_t n_digests) const {
    SA_HIP_CHECK_DRAIN(s, hipMemcpyAsync(pin + l.meta, dev + l.meta, l.result - l.meta + n * 8,
                                         hipMemcpyDeviceToHost, s));
    SA_HIP_CHECK_DRAIN(s, hipStreamSynchronize(s));
    memcpy(out, pin + l.result, n * 8);
    const uint64_t* meta = (const uint64_t*)(pin + l.meta);
    if (flags) *flags = (uint32_t)*meta++;
    if (digests) memcpy(digests, meta, n_digests * 8);
    return SA_OK;
  }
};

}  // namespace

extern "C" int sa_fused_clients_host_f32(const float* const* host_x, const double* weights, int n_clients,
                                         uint64_t n, int fxp_bits, const sa_pcg64* pair_gens,
                                         const int8_t* pair_sign, double divisor, void* pinned, void* dev,
                                         double* out, uint64_t* digests, uint32_t* flags, void* stream) {
  if (!host_x || !weights || n_clients < 2 || n_clients > 8 || n == 0 || !pair_gens || !pair_sign || !out ||
      !digests || !flags || !scratch_ok(pinned, dev)) {
    sa_set_error("sa_fused_clients_host_f32: bad arguments (2..8 clients, n > 0, 16-byte aligned buffers)");
    return SA_ERR_ARG;
  }
  if (check_vectors((const void* const*)host_x, n_clients, "sa_fused_clients_host_f32", "host_x"))
    return SA_ERR_ARG;
  const uint64_t C = (uint64_t)n_clients;
  const HostCall h(fused_host_layout(C, n), pinned, dev, stream);
  int rc = h.upload((const void* const*)host_x, C, n * 4);
  if (rc) return rc;
  sa_local_client cl[8];
  for (uint64_t c = 0; c < C; c++) {
    cl[c].x = h.d_in(c);
    cl[c].weight = weights[c];
    cl[c].masked_out = nullptr;
  }
  uint64_t* d_sum = h.d_tail();
  rc = sa_fused_clients(cl, n_clients, SA_F32, n, fxp_bits, pair_gens, pair_sign, nullptr, 0, d_sum, 0,
                        h.d_meta() + 1, (uint32_t*)h.d_meta(), stream);
  if (rc) return drain(h.s, rc);
  rc = sa_decode(d_sum, n, fxp_bits, divisor, nullptr, (double*)h.d_result(), stream);
  if (rc) return drain(h.s, rc);
  return h.finish(n, out, flags, digests, C);
}

extern "C" int sa_clients_host(const void* const* host_x, int x_type, int compute_type, const double* weights,
                               int n_clients, uint64_t n, int fxp_bits, const sa_mask_stream* streams,
                               double divisor, void* pinned, void* dev, double* out, uint64_t* digests,
                               uint32_t* flags, void* stream) {
  if (check_type(x_type, "sa_clients_host x_type") || check_type(compute_type, "sa_clients_host compute_type"))
    return SA_ERR_ARG;
  if (!host_x || !weights || n_clients < 2 || n_clients > 9 || n == 0 || !streams || !out || !digests || !flags ||
      !scratch_ok(pinned, dev)) {
    sa_set_error("sa_clients_host: bad arguments (2..9 clients, n > 0, 16-byte aligned buffers)");
    return SA_ERR_ARG;
  }
  if (check_vectors(host_x, n_clients, "sa_clients_host", "host_x")) return SA_ERR_ARG;
  const uint64_t C = (uint64_t)n_clients, xs = x_type == SA_F32 ? 4 : 8;
  const HostCall h(clients_host_layout(C, n, xs), pinned, dev, stream);
  int rc = h.upload(host_x, C, n * xs);
  if (rc) return rc;
  uint64_t* d_sum = h.d_zeroed();
  for (uint64_t c = 0; c < C; c++) {
    rc = sa_mask(h.d_in(c), x_type, compute_type, n, weights[c], nullptr, fxp_bits, streams + c * (C - 1),
                 n_clients - 1, h.d_tail() + c * n_pad(n), d_sum, h.d_meta() + 1 + c, (uint32_t*)h.d_meta(), stream);
    if (rc) return drain(h.s, rc);
  }
  rc = sa_decode(d_sum, n, fxp_bits, divisor, nullptr, (double*)h.d_result(), stream);
  if (rc) return drain(h.s, rc);
  return h.finish(n, out, flags, digests, C);
}

extern "C" int sa_mask_host(const void* host_x, int x_type, int compute_type, uint64_t n, double weight,
                            int fxp_bits, const sa_mask_stream* streams, int n_streams, void* pinned, void* dev,
                            uint64_t* out, uint32_t* flags, void* stream) {
  if (check_type(x_type, "sa_mask_host x_type") || check_type(compute_type, "sa_mask_host compute_type"))
    return SA_ERR_ARG;
  if (!host_x || n == 0 || n_streams < 0 || (n_streams > 0 && !streams) || !out || !flags ||
      !scratch_ok(pinned, dev)) {
    sa_set_error("sa_mask_host: bad arguments (n > 0, 16-byte aligned buffers)");
    return SA_ERR_ARG;
  }
  const uint64_t xs = x_type == SA_F32 ? 4 : 8;
  const HostCall h(mask_host_layout(n, xs), pinned, dev, stream);
  int rc = h.upload(&host_x, 1, n * xs);
  if (rc) return rc;
  rc = sa_mask(h.d_in(0), x_type, compute_type, n, weight, nullptr, fxp_bits, streams, n_streams,
               (uint64_t*)h.d_result(), nullptr, nullptr, (uint32_t*)h.d_meta(), stream);
  if (rc) return drain(h.s, rc);
  return h.finish(n, out, flags, nullptr, 0);
}

extern "C" int sa_sum_decode_host(const uint64_t* const* host_masked, int n_clients, uint64_t n, int fxp_bits,
                                  double divisor, void* pinned, void* dev, double* out, uint64_t* digests,
                                  void* stream) {
  if (!host_masked || n_clients < 1 || n_clients > kSumMaxIn || n == 0 || !out || !digests ||
      !scratch_ok(pinned, dev)) {
    sa_set_error("sa_sum_decode_host: bad arguments (1..%d vectors, n > 0, 16-byte aligned buffers)", kSumMaxIn);
    return SA_ERR_ARG;
  }
  if (check_vectors((const void* const*)host_masked, n_clients, "sa_sum_decode_host", "host_masked"))
    return SA_ERR_ARG;
  const uint64_t C = (uint64_t)n_clients;
  const HostCall h(sum_decode_host_layout(C, n), pinned, dev, stream);
  int rc = h.upload((const void* const*)host_masked, C, n * 8);
  if (rc) return rc;
  const uint64_t* ins[kSumMaxIn];
  for (uint64_t c = 0; c < C; c++) {
    ins[c] = (const uint64_t*)h.d_in(c);
    rc = sa_xor_u64(ins[c], n, h.d_meta() + c, stream);
    if (rc) return drain(h.s, rc);
  }
  uint64_t* d_sum = h.d_tail();
  rc = sa_sum_u64(ins, n_clients, n, d_sum, stream);
  if (rc) return drain(h.s, rc);
  rc = sa_decode(d_sum, n, fxp_bits, divisor, nullptr, (double*)h.d_result(), stream);
  if (rc) return drain(h.s, rc);
  return h.finish(n, out, nullptr, digests, C);
}
