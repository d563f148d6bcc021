// sa_host_layout.h — scratch layout of the four blocking host-array entries
// (sa_host_calls.hip).  Plain C++, no HIP: tests/test_boundary.py compiles it
// with the host compiler against the sizes sfl_amd/kernels.py advertises.
//
// All four lay the pinned and the device scratch out alike:
//
//   [ inputs: n_vec x n_pad elements | sum: n_pad u64 (sa_clients_host only) |
//     meta words: flag and/or digests | result: n_pad 8-B elements ]
//   (+ device only: the tail)
//
// so that the words the kernels accumulate into (PRG flag, digests, and for
// sa_clients_host the masked sum) ride the one host-to-device copy as zeros
// -- no separate fill -- and the words read back sit right before the
// result, so one device-to-host copy brings everything (a small call is
// bound by its number of device operations).
#pragma once
#include <stdint.h>

namespace sa {

// vectors are staged n_pad elements apart, so every one starts 16-B aligned
inline uint64_t n_pad(uint64_t n) { return (n + 3) & ~3ull; }
// the meta words end 16-B aligned: an even count of 8-B words
inline uint64_t even_words(uint64_t w) { return (w + 1) & ~1ull; }
// sa_clients_host: a sum of up to 16 KiB rides the copy as zeros, a larger one is filled on the device
constexpr uint64_t kZeroByCopyMax = 16u << 10;

// byte offsets into the pinned and the device scratch (the same in both)
struct HostLayout {
  uint64_t in_stride;     // staged input c at c * in_stride
  uint64_t zeroed;        // start of the words that must be zero on the device: the sum if there is one, else meta
  uint64_t meta;          // the meta words
  uint64_t result;        // the result; everything before it is uploaded, meta and result come back
  uint64_t tail;          // device-only words (== pinned_bytes)
  uint64_t pinned_bytes, dev_bytes;
  bool zero_by_copy;      // the zeroed words ride the upload; else: a device fill after it
};

// n_vec vectors of n elements of elem_size bytes, sum_words 8-B words ahead
// of meta_words meta words, tail_words device-only 8-B words
inline HostLayout host_layout(uint64_t n_vec, uint64_t n, uint64_t elem_size, uint64_t sum_words,
                              uint64_t meta_words, uint64_t tail_words) {
  HostLayout l;
  l.in_stride = n_pad(n) * elem_size;
  l.zeroed = n_vec * l.in_stride;
  l.meta = l.zeroed + sum_words * 8;
  l.result = l.meta + even_words(meta_words) * 8;
  l.tail = l.pinned_bytes = l.result + n_pad(n) * 8;
  l.dev_bytes = l.tail + tail_words * 8;
  l.zero_by_copy = sum_words * 8 <= kZeroByCopyMax;
  return l;
}

// sa_fused_clients_host_f32: meta = flag, a digest per client; tail = the masked sum
inline HostLayout fused_host_layout(uint64_t n_clients, uint64_t n) {
  return host_layout(n_clients, n, 4, 0, 1 + n_clients, n_pad(n));
}
// sa_clients_host: the masked sum ahead of meta = flag, a digest per client; tail = every client's masked vector
inline HostLayout clients_host_layout(uint64_t n_clients, uint64_t n, uint64_t elem_size) {
  return host_layout(n_clients, n, elem_size, n_pad(n), 1 + n_clients, n_clients * n_pad(n));
}
// sa_mask_host: meta = flag word + pad; result = the masked vector; no tail
inline HostLayout mask_host_layout(uint64_t n, uint64_t elem_size) { return host_layout(1, n, elem_size, 0, 2, 0); }
// sa_sum_decode_host: meta = a digest per vector; tail = the sum
inline HostLayout sum_decode_host_layout(uint64_t n_clients, uint64_t n) {
  return host_layout(n_clients, n, 8, 0, n_clients, n_pad(n));
}

}  // namespace sa
