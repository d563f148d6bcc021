/*
 * sfl_sa.h — C-ABI of the MI355X secure-aggregation hot path (libsfl_sa.so).
 *
 * Drop-in boundary for the element-wise core of
 * secretflow.security.aggregation.SecureAggregator (un-vendored dependency
 * secretflow-lite==1.13.0b0, /root/reference/pyproject.toml:51).  Each entry
 * point below cites the reference interface it replaces.  Python reaches it
 * through ctypes (sfl_amd/_lib.py); INTEGRATION.md shows the binding a
 * maintainer would add on the reference side.
 *
 * Conventions
 *  - every function returns int: SA_OK (0) or a negative SA_ERR_* code; no
 *    exception crosses the ABI.  sa_last_error() returns a message.
 *  - device buffers are caller-owned; launches are asynchronous and ordered
 *    on the caller's hipStream_t (passed as void*; NULL = legacy stream).
 *  - the launch functions never allocate, copy or synchronise, so they can be
 *    captured into a hipGraph.  Re-entrant per stream.  The four *_host
 *    entries are the exception: blocking calls on host arrays for small
 *    payloads (they copy and synchronise, but allocate nothing either).
 *  - n == 0 is a no-op that returns SA_OK; the vector pointers of an empty
 *    call may be NULL (an empty framework tensor has no storage).
 *  - mask-stream generator states are numpy PCG64 states (state, inc) as
 *    128-bit little-endian pairs; the caller advances them between rounds
 *    with sa_pcg64_advance(), exactly like the reference's persistent
 *    np.random.Generator objects advance by one draw per masked element.
 */
#ifndef SFL_SA_H
#define SFL_SA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SA_ABI_VERSION 3

/* status codes */
#define SA_OK 0
#define SA_ERR_ARG (-1)         /* bad argument (null pointer, size, unsupported combo) */
#define SA_ERR_HIP (-2)         /* HIP runtime error */
#define SA_ERR_UNSUPPORTED (-3) /* valid request this build has no kernel for */
#define SA_ERR_RCCL (-4)        /* RCCL error */

/* element types */
#define SA_F32 0
#define SA_F64 1
#define SA_I64 2

/* bits set in *flags by the kernels */
#define SA_FLAG_PRG_REJECT 1u /* a PCG64 raw draw was 0: numpy's Lemire bounded
                                 draw would have rejected it and re-drawn (p=2^-64
                                 per draw).  The mask stream then differs from
                                 numpy's from that element on; the host
                                 re-positions it (sa_pcg64_find_zero,
                                 sa_stream_shift, sa_xor_u64 below). */

typedef struct sa_u128 {
  uint64_t lo, hi;
} sa_u128;

/* numpy PCG64 bit_generator.state['state'] = {state, inc} */
typedef struct sa_pcg64 {
  sa_u128 state;
  sa_u128 inc;
} sa_pcg64;

/* One pairwise mask stream as seen by ONE client (the owner of the stream
 * for this call).  sign = +1 when the peer's name sorts after the client's
 * (q += m), -1 otherwise (q -= m): the `party > self._party` rule of the
 * masking equation, docs/developer/algorithm/secure_aggregation.ipynb
 * cell 15. */
typedef struct sa_mask_stream {
  sa_pcg64 gen; /* generator state before draw 0 of this call */
  int32_t sign; /* +1 / -1 */
  int32_t peer; /* informational (peer client index) */
} sa_mask_stream;

/* A client co-located on this GPU for the fused kernel. */
typedef struct sa_local_client {
  const void* x;        /* n elements of x_type, device pointer */
  double weight;        /* scalar weight w_c (1.0 = none); applied in the compute type */
  uint64_t* masked_out; /* optional: this client's masked vector (wire image), n u64 */
} sa_local_client;

/* ------------------------------------------------------------------ */
/* library / setup (host only, no GPU needed)                          */
/* ------------------------------------------------------------------ */

int sa_abi_version(void);
const char* sa_last_error(void);

/* numpy.random.PCG64(seed) seeding: SeedSequence(entropy) -> generate_state(4,
 * uint64) -> pcg_setseq_128_srandom.  `words` is the entropy as 32-bit
 * little-endian words (numpy's _coerce_to_uint32_array of a non-negative int).
 * Replaces: `np.random.default_rng(seed)` inside the un-vendored _Masker
 * (secure_aggregation.ipynb cell 15 names numpy.random.PCG64). */
int sa_pcg64_from_seed(const uint32_t* words, int n_words, sa_pcg64* out);

/* == numpy PCG64.advance(delta): jump the generator by delta draws. */
int sa_pcg64_advance(sa_pcg64* g, sa_u128 delta);

/* out[i] = in[i] advanced by delta[i] draws, for count generators in one
 * call (the per-round positioning of a party's pair streams: one call per
 * round instead of one per stream; out may alias in). */
int sa_pcg64_advance_many(const sa_pcg64* in, const uint64_t* delta, int count, sa_pcg64* out);

/* Host-side reference draws, for validating the seeding/jump math only
 * (tests).  Not used by any hot-path entry point. */
int sa_pcg64_raw_host(sa_pcg64* g, uint64_t* out, uint64_t n);

/* ------------------------------------------------------------------ */
/* hot path (device, asynchronous on `stream`)                          */
/* ------------------------------------------------------------------ */

/* _Masker.mask for ONE client (un-vendored; equation at
 * secure_aggregation.ipynb cell 15, quantizer pinned by the KAT of cells
 * 17-18): masked[i] = trunc(x[i]*w*2^fxp) + sum_j sign_j * m_j[i]  (mod 2^64),
 * m_j = PCG64(gen_j).integers(int64.min, int64.max, n).astype(uint64).
 *
 *   x, x_type       input vector (SA_F32/SA_F64/SA_I64).  x == NULL means
 *                   "continue": start from the current contents of `out`
 *                   (multi-pass masking when n_streams exceeds one pass).
 *   compute_type    arithmetic type of x*w*2^fxp (numpy promotion result:
 *                   SA_F32 for float32 data with a python-scalar weight,
 *                   SA_F64 for float64 data or array weights, SA_I64 for
 *                   integer data and weights).
 *   weight          scalar weight (1.0 = none)
 *   weight_vec      optional per-element weights (n elements, compute_type)
 *   out             masked vector, n u64 (required)
 *   sum_accum       optional: sum_accum[i] += masked[i]
 *   digest          optional: *digest ^= XOR of all masked[i]
 *   flags           optional: |= SA_FLAG_*
 */
int sa_mask(const void* x, int x_type, int compute_type, uint64_t n, double weight,
            const void* weight_vec, int fxp_bits, const sa_mask_stream* streams, int n_streams,
            uint64_t* out, uint64_t* sum_accum, uint64_t* digest, uint32_t* flags, void* stream);

/* Fused single-GPU simulation of C = n_clients co-located clients (config 2
 * and the 1-GPU headline): quantize every client, expand every internal pair
 * stream ONCE and apply it +/- to both of its clients, apply each client's
 * n_cross cross-GPU streams, and write the masked sum.  Each client's masked
 * vector is formed in registers: it is XOR-folded into digests[c] and, when
 * clients[c].masked_out != NULL, stored (wire image).
 *
 *   pair_gens       n_clients*(n_clients-1)/2 generators, pair (u<v) at
 *                   index u*(2C-u-1)/2 + (v-u-1)
 *   pair_sign       +1 when client u adds the pair mask (name_v > name_u)
 *   cross           n_clients * n_cross streams, client-major
 *   sum_out         n u64; accumulate != 0 means sum_out[i] += local sum
 *   digests         n_clients u64 (XOR-accumulated; zero them first)
 * More than 32 streams with only the sum wanted (no digests, no masked_out;
 * float32; e.g. 32 clients, 4 per GPU: 6 pairs + 4 x 28 cross streams): a
 * multi-launch schedule on the same stream -- one fused launch with the
 * internal pairs (each still expanded once) and the first cross streams,
 * then masks-only launches of the remaining cross streams into sum_out.
 * Other shapes without a fused kernel (more than 8 clients, more than 32
 * streams with digests or wire images, or an uninstantiated (C, n_cross))
 * return SA_ERR_UNSUPPORTED: the caller then masks client by client with
 * sa_mask(..., sum_accum), same result, or -- more than 8 clients, only
 * the sum wanted -- runs the pair-shared schedule with sa_fused_bipartite.
 * Replaces: the client-side `mask` calls plus server `_sum`'s
 * np.sum(..., axis=0) for co-located parties. */
int sa_fused_clients(const sa_local_client* clients, int n_clients, int x_type, uint64_t n,
                     int fxp_bits, const sa_pcg64* pair_gens, const int8_t* pair_sign,
                     const sa_mask_stream* cross, int n_cross, uint64_t* sum_out, int accumulate,
                     uint64_t* digests, uint32_t* flags, void* stream);

/* Host-resident float32 clients, co-located on one GPU, in ONE blocking call:
 * the small-call path of `SecureAggregator.sum` / `.average` on host arrays
 * (FL rounds of small models, HomoBinning's
 * counts), where per-call latency, not bandwidth, decides.  Copies the
 * n_clients host vectors into `pinned`, ONE host-to-device copy (inputs and
 * zeroed flag + digest words), sa_fused_clients (masked_out NULL, no cross streams),
 * sa_decode by `divisor`, ONE device-to-host copy of result + flag word +
 * digests, synchronises `stream`, then fills the outputs (the zeroed flag
 * and digest words ride the host-to-device copy: no fill operation).  With
 * n_pad = n rounded up to a multiple of 4 and M = 1 + n_clients rounded up
 * to even, the caller owns (nothing is allocated):
 *   pinned  >= n_clients*n_pad*4 + (M + n_pad)*8 bytes of page-locked host
 *           memory, 16-byte aligned;
 *   dev     >= n_clients*n_pad*4 + (M + 2*n_pad)*8 bytes of device memory,
 *           16-byte aligned.
 * Outputs (host): out[n] the decoded float64, digests[n_clients] the masked
 * vectors' XOR digests, *flags the PRG flag word (SA_FLAG_PRG_REJECT: the
 * caller replays the round as after sa_fused_clients).  2..8 clients.
 * Unlike the launch functions this one blocks: it returns once the result
 * is on the host.  Replaces, for co-located parties, the per-party `mask`
 * calls plus the server's `_sum` and decode. */
int sa_fused_clients_host_f32(const float* const* host_x, const double* weights, int n_clients, uint64_t n,
                              int fxp_bits, const sa_pcg64* pair_gens, const int8_t* pair_sign, double divisor,
                              void* pinned, void* dev, double* out, uint64_t* digests, uint32_t* flags,
                              void* stream);

/* The same blocking small call for any element type (float64 / int64 data,
 * or float32 data with a float64 compute type): n_clients host vectors of
 * x_type, every party masked by sa_mask with its OWN streams (no pair
 * sharing: the non-float32 kernels hold one client) into a zeroed masked
 * sum, then sa_decode.  `streams`: n_clients * (n_clients - 1) entries,
 * client-major (client c's peers in its masker's order); `weights` are the
 * scalar weights as sa_mask takes them.  With n_pad = n rounded up to a
 * multiple of 4, xs the element size of x_type and M = 1 + n_clients
 * rounded up to even:
 *   pinned >= n_clients*n_pad*xs + (2*n_pad + M)*8 bytes, page-locked;
 *   dev    >= n_clients*n_pad*(xs + 8) + (2*n_pad + M)*8 bytes;
 * both 16-byte aligned.  2..9 clients.  Outputs as for
 * sa_fused_clients_host_f32.  Replaces, for co-located parties with small
 * integer / float64 vectors (HomoBinning's counts),
 * the per-party `mask` calls plus the server's `_sum` and decode. */
int sa_clients_host(const void* const* host_x, int x_type, int compute_type, const double* weights,
                    int n_clients, uint64_t n, int fxp_bits, const sa_mask_stream* streams, double divisor,
                    void* pinned, void* dev, double* out, uint64_t* digests, uint32_t* flags, void* stream);

/* The per-party drop-in's two device steps for small host payloads, each as
 * ONE blocking call (sfl_amd/security/aggregation/party.py; the reference's
 * `_Masker.mask` inside the participant and the server's `_sum` + decode,
 * secure_aggregation.ipynb:227-239, sparse_plain_aggregator.py:86-94).
 *
 * sa_mask_host: one party's masked vector.  Copies host_x (n elements of
 * x_type) into `pinned`, one host-to-device copy, zeroes the flag word,
 * sa_mask with `streams`, one device-to-host copy of the masked vector and
 * the flag word, synchronises, fills out[n] (host) and *flags.  n_pad = n
 * rounded up to a multiple of 4, xs = element size:
 *   pinned >= n_pad*xs + (2 + n_pad)*8 bytes, page-locked;  dev >= the same. */
int sa_mask_host(const void* host_x, int x_type, int compute_type, uint64_t n, double weight, int fxp_bits,
                 const sa_mask_stream* streams, int n_streams, void* pinned, void* dev, uint64_t* out,
                 uint32_t* flags, void* stream);

/* sa_sum_decode_host: the server's step.  Copies the n_clients host masked
 * vectors into `pinned`, one host-to-device copy, each vector's XOR digest,
 * their sum mod 2^64, decode by `divisor`, one device-to-host copy of the
 * result and the digests, synchronises, fills out[n] and digests[n_clients]
 * (host; the caller compares them with the digests the parties sent).
 * With M = n_clients rounded up to even:
 *   pinned >= (n_clients*n_pad + M + n_pad)*8 bytes, page-locked;
 *   dev    >= (n_clients*n_pad + M + 2*n_pad)*8 bytes;
 * 1..32 vectors, both buffers 16-byte aligned. */
int sa_sum_decode_host(const uint64_t* const* host_masked, int n_clients, uint64_t n, int fxp_bits, double divisor,
                       void* pinned, void* dev, double* out, uint64_t* digests, void* stream);

/* One block of the pair-shared schedule for MORE co-located clients than one
 * sa_fused_clients launch holds (more than 8): the 8 slots are two quads of
 * clients, (0-3) and (4-7), and the launch expands only the 16 streams of the
 * pairs BETWEEN the quads, each once, applied to both clients (pair_gens /
 * pair_sign a-major: pair p = (p / 4, 4 + p % 4); sign for the lower slot as
 * in sa_fused_clients).  Masks only: the slots' x and masked_out must be
 * NULL (the clients' quantized values, and each quad's internal pairs, come
 * from a sa_fused_clients launch over the clients of two quads); the 16
 * masks, added to both clients of each pair, go straight into the sum
 * (sum_out = or += their sum), so every pair stream of C clients is expanded
 * exactly once:
 * C(C-1)/2 draws per element instead of C(C-1) (sfl_amd/kernels.py
 * fused_many).  Replaces the per-party `_Masker.mask` + server sum of
 * SURVEY 8a a2-a5 for simulations with many parties per GPU.  float32 only. */
int sa_fused_bipartite(const sa_local_client* clients, int x_type, uint64_t n, int fxp_bits,
                       const sa_pcg64* pair_gens, const int8_t* pair_sign, uint64_t* sum_out,
                       int accumulate, uint32_t* flags, void* stream);

/* Host setting for this process's masking launches (sa_mask, sa_fused_*):
 * leave `cus` CUs' worth of the kernel's occupancy free for kernels that run
 * concurrently on other streams -- the RCCL exchange of the previous chunk
 * in the pipelined multi-GPU path, whose kernels otherwise wait for the
 * masking grid (occupancy-sized, it fills every CU) to drain.  0 (default):
 * the whole GPU.  At most half of the occupancy is ever reserved.  Results
 * are unchanged (the grid only decides which tiles a block takes). */
int sa_set_masking_reserve(int cus);

/* Server `_sum`: out[i] = sum_k in[k][i] mod 2^64 (np.sum over uint64,
 * pattern of sfl/security/aggregation/sparse_plain_aggregator.py:88-94).
 * `in` is a HOST array of k device pointers; out may alias in[0]. */
int sa_sum_u64(const uint64_t* const* in, int k, uint64_t n, uint64_t* out, void* stream);

/* Server decode: out[i] = (double)(int64)s[i] / 2^fxp / div, with
 * div = divisor_vec[i] when divisor_vec != NULL (per-element weights,
 * CHANGELOG.md:994) else `divisor` (1.0 for sum, C or sum(w) for average).
 * Division is IEEE (correctly rounded), matching numpy float64.  16-byte
 * aligned s / out / divisor_vec take 16-B accesses (two elements per lane),
 * other alignments one 8-B element per lane. */
int sa_decode(const uint64_t* s, uint64_t n, int fxp_bits, double divisor,
              const double* divisor_vec, double* out, void* stream);

/* Element-wise sum of per-client weight arrays for per-element-weight
 * averages: out[i] = sum_k w[k][i] (float64), `w` a HOST array of k device
 * pointers.  16-B accesses when every buffer is 16-byte aligned. */
int sa_sum_f64(const double* const* w, int k, uint64_t n, double* out, void* stream);

/* ------------------------------------------------------------------ */
/* numpy's rejection re-draw, reproduced after a SA_FLAG_PRG_REJECT     */
/* (never on the hot path).  Generator.integers(int64.min, int64.max)   */
/* rejects a raw PCG64 output of 0 and takes the next one, so from that */
/* element on the stream runs one raw draw further along.  A pair       */
/* stream enters its two clients with opposite signs: the masked SUM is */
/* unchanged, only per-client masked vectors and digests move.          */
/* ------------------------------------------------------------------ */

/* first_out[j] = min(first_out[j], smallest i in [0, n) whose raw draw i of
 * gens[j] (the output after i + 1 steps) is 0).  `gens` is a HOST array;
 * first_out is device memory the caller fills with UINT64_MAX first. */
int sa_pcg64_find_zero(const sa_pcg64* gens, int n_gens, uint64_t n, uint64_t* first_out, void* stream);

/* out[e] += sign * (raw[e + shift] - raw[e + shift - 1])  (mod 2^64) for e in
 * [k, n), raw relative to `gen` (raw[0] = the first step's output): moves a
 * masked vector that used raw[e + shift - 1] for element e onto
 * raw[e + shift] (the mask offset K cancels in the difference). */
int sa_stream_shift(uint64_t* out, uint64_t n, const sa_pcg64* gen, int sign, uint64_t k, uint64_t shift,
                    void* stream);

/* *digest ^= XOR of v[0..n) (the per-client digest of sa_fused_clients). */
int sa_xor_u64(const uint64_t* v, uint64_t n, uint64_t* digest, void* stream);

/* ------------------------------------------------------------------ */
/* GaussianModelDP pre-step (sfl/security/privacy/mechanism/            */
/* mechanism_fl.py:62-130), applied by a client before masking:         */
/*   x' = x * min(1, clip / ||x||) + N(0, sigma^2) / num_updates        */
/* in float32, sigma = noise_multiplier * clip * clip as the reference  */
/* computes it.  ||x|| is the global norm over all layers (or, with     */
/* sumsq_layer, min(1, clip / sqrt(||layer|| * ||all||)) per layer,     */
/* is_clip_each_layer).  The noise is Philox4x32-10 + Box-Muller keyed   */
/* by (key, element index), not numpy's unseeded global MT19937 stream:  */
/* parity for the noise is distributional; the clip follows the         */
/* reference's float32 norm arithmetic (sa_sumsq_f32), up to its BLAS    */
/* dot's float32 accumulation order.                                     */
/* ------------------------------------------------------------------ */

#define SA_DP_PARTIALS 1024 /* doubles of scratch for sa_sumsq_f32 */

typedef struct sa_dp {
  const double* sumsq;       /* device: the clipping group's squared norm (sa_sumsq_f32) */
  const double* sumsq_layer; /* device, optional: this layer's squared norm */
  double l2_norm_clip;       /* the reference's python float (the clip divides in float64) */
  float noise_std;   /* sigma */
  float num_updates; /* divisor of the noise (> 0) */
  uint64_t key;      /* Philox key */
  uint64_t counter0; /* noise index of element 0 (multiple of 4) */
} sa_dp;

/* *sumsq (+)= this layer's squared L2 norm as the reference forms it under
 * its numpy 1.23.5 (mechanism_fl.py:132-135 on float32 arrays):
 * np.linalg.norm is a float32 dot and a float32 sqrt (here the dot is the
 * deterministic fixed-order float64 sum of x[i]^2 rounded once to float32;
 * the reference's BLAS sdot adds in float32 in its own order);
 * `** 2` of that float32 scalar with a python int is float64 in numpy 1.x
 * (scalar-scalar operations promote without value-based casting), so the
 * square is exact; python's sum adds the layers in float64 from 0.
 * `partials` is caller scratch of SA_DP_PARTIALS doubles.  ABI version 3. */
int sa_sumsq_f32(const float* x, uint64_t n, double* partials, double* sumsq, int accumulate, void* stream);

/* out = clip-and-noise(x) (out may alias x). */
int sa_dp_perturb_f32(const float* x, uint64_t n, const sa_dp* dp, float* out, void* stream);

/* sa_mask of the DP-perturbed float32 x without materialising it: the
 * clip+noise runs inside the masking kernel on the loaded tile.  Equal bit
 * for bit to sa_dp_perturb_f32 followed by sa_mask. */
int sa_mask_dp(const float* x, uint64_t n, double weight, int fxp_bits, const sa_mask_stream* streams,
               int n_streams, const sa_dp* dp, uint64_t* out, uint64_t* sum_accum, uint64_t* digest,
               uint32_t* flags, void* stream);

/* ------------------------------------------------------------------ */
/* multi-GPU exchange: the masked-sum reduce over RCCL (xGMI)           */
/* Replaces the RayFed `.to(server)` transfer + server np.sum           */
/* (sfl/distributed/op_strategy.py:131-141; sparse_plain_aggregator.py:86) */
/* ------------------------------------------------------------------ */

#define SA_UNIQUE_ID_BYTES 128

int sa_comm_unique_id(void* id_out, int cap);
int sa_comm_init(void** comm, const void* id, int nranks, int rank, int device);
/* ncclReduce(ncclUint64, ncclSum): recv (on root) = sum over ranks of send.
 * Bit-exact for any RCCL algorithm: uint64 add is associative mod 2^64.
 * recv may be NULL on non-root ranks: the reduce then runs in place on send
 * (the call pattern torch.distributed.reduce uses), never on a null buffer. */
int sa_comm_reduce_u64(void* comm, const uint64_t* send, uint64_t* recv, uint64_t n, int root,
                       void* stream);
int sa_comm_allreduce_u64(void* comm, const uint64_t* send, uint64_t* recv, uint64_t n,
                          void* stream);
/* The sharded server (SURVEY.md §8(e) "ReduceScatter, then decode the shards
 * in parallel, then Gather float64"): ncclReduceScatter(ncclUint64, ncclSum),
 * rank r's recv (count elements) = sum over ranks of send[r*count, (r+1)*count);
 * in place when recv == send + r*count.  Same exchange as sa_comm_reduce_u64
 * (the server's np.sum, sparse_plain_aggregator.py:88-94), the server split
 * over the ranks. */
int sa_comm_reduce_scatter_u64(void* comm, const uint64_t* send, uint64_t* recv, uint64_t count,
                               void* stream);
/* The sharded server's exchange as direct transfers (each shard crosses one
 * point-to-point xGMI link): for every rank p != r, rank r's recv[p*count,
 * (p+1)*count) = rank p's send[r*count, (r+1)*count) (grouped ncclSend /
 * ncclRecv); recv's slot r is not written.  The caller sums the shards with
 * sa_sum_u64 (its own shard from send): the same result and wire bytes as
 * sa_comm_reduce_scatter_u64, without RCCL's reduce schedule. */
int sa_comm_alltoall_u64(void* comm, const uint64_t* send, uint64_t* recv, uint64_t count,
                         void* stream);
/* The decoded float64 shards to the server: on root, recv[r*count, (r+1)*count)
 * = rank r's send (grouped ncclSend/ncclRecv); recv may be NULL off root. */
int sa_comm_gather_f64(void* comm, const double* send, double* recv, uint64_t count, int root,
                       void* stream);
/* What RCCL made of the communicator (ncclCommCount, ncclCommUserRank,
 * ncclCommCuDevice): the bench line's `rccl` record, so a scaling run shows
 * by itself that RCCL saw N ranks on N devices.  Any pointer may be NULL. */
int sa_comm_info(void* comm, int* nranks, int* rank, int* device);
int sa_comm_destroy(void* comm);

/* ------------------------------------------------------------------ */
/* Sparse ternary compression (fed_stc): the reference's STCSparse      */
/* (sfl/utils/compressor/sparse_compressor.py:142-179) with the error   */
/* feedback around it, on a worker (new - old + residual, sfl/ml/nn/fl/ */
/* backend/torch/strategy/fed_stc.py:97-125) and on the server          */
/* (aggregate + residual, server weights += sparse, sfl/ml/nn/fl/       */
/* compress.py:28-42; fl_model.py:542-563).  For n elements of x_type   */
/* T (SA_F32 or SA_F64), every operation rounded in T:                  */
/*   u      = (a - b) + r          b, r optional: absent = not performed */
/*   masked = the mask_num elements of smallest |u|, ordered by the bit */
/*            pattern of |u| as an unsigned integer (numpy's order, NaN */
/*            last); equal keys: the lower index is masked first        */
/*            (np.argsort(kind="stable"); the reference's default sort  */
/*            breaks such ties arbitrarily)                             */
/*   mu     = T(S / (n - mask_num)), S the float64 sum of the survivors' */
/*            |u| in an order that depends on n only (no float atomics: */
/*            the same input gives the same bits); 0 when mask_num == n */
/*   sparse_out = mu * sign(u_masked)   (a real multiply: NaN and inf   */
/*            propagate as in numpy)                                    */
/*   res_out    = u - sparse_out        (may alias r; nothing else may  */
/*            alias)                                                    */
/*   acc_inout += sparse_out            (optional: the server's weights) */
/* A radix select on the key finds the threshold (no sort); threshold,  */
/* tie quota and mu stay in device memory.  mu_out (optional) is one T  */
/* on the device.  n >= 2^32 and other element types are refused.       */
/* 16-byte aligned vectors take 16-byte loads and stores.               */
/* ------------------------------------------------------------------ */

/* bytes of device scratch sa_stc needs for n elements (8-byte aligned, its
 * content is rewritten by every call), or a negative SA_ERR_* code */
int sa_stc_scratch_bytes(uint64_t n, int x_type);

int sa_stc(const void* a, const void* b, const void* r, int x_type, uint64_t n, uint64_t mask_num,
           void* sparse_out, void* res_out, void* acc_inout, void* mu_out, void* scratch, void* stream);

/* ------------------------------------------------------------------ */
/* Structure-wise update pruning (fed_scr): the reference's SCRSparse   */
/* (sfl/utils/compressor/sparse_compressor.py:182-230) with the update  */
/* and the residual of a worker around it (sfl/ml/nn/fl/backend/torch/  */
/* strategy/fed_scr.py:97-125).  A dense layer [R, C] is the tensor     */
/* [rows, cols, 1], a conv layer [O, I, H, W] is [O, I, H*W].  For      */
/* n = rows*cols*inner elements of x_type T (SA_F32 or SA_F64) and a    */
/* double threshold:                                                   */
/*   u      = (a - b) + r          every operation rounded in T; b, r   */
/*            optional: absent = not performed                          */
/*   S0[i]  = float64 sum of |u[i,:,:]|;  M0 = max(S0), NaN propagating */
/*            (np.max); row i is dropped iff S0[i] / M0 <= threshold, a */
/*            real float64 division and comparison                      */
/*   S1[j]  = float64 sum of |u[i,j,:]| over the KEPT rows i;  M1 and   */
/*            the rule as for rows                                      */
/*   sparse_out = u with the dropped rows and columns +0.0; a kept      */
/*            element keeps its bits (-0.0, NaN payloads)               */
/*   res_out    = u - sparse_out, a real subtraction in T (optional;    */
/*            may alias r; nothing else may alias)                      */
/*   stats_out  = two uint32 on the device: dropped rows, dropped       */
/*            columns (optional)                                        */
/* The special cases are IEEE's, as in numpy: an all-zero tensor (0/0)  */
/* and a tensor with a NaN (M NaN) drop nothing; a row with an inf has  */
/* ratio inf/inf = NaN and is kept while the finite rows have ratio 0;  */
/* a negative threshold drops nothing; when every row is dropped S1 is  */
/* all zero and no column is.                                           */
/* The one refinement against the reference: decisions are taken on     */
/* float64 sums and ratios, the reference's on T's.  For float32 data   */
/* the two can differ only where a ratio lies within rounding (about    */
/* 1e-6 relative) of the threshold.                                     */
/* The sums are added in an order that depends on the shape only (no    */
/* float atomics): the same input gives the same bits on every run.     */
/* Maxima, flags and counts stay in device memory; nothing is allocated */
/* or synchronised.  n >= 2^32, a zero dimension, other element types   */
/* and a shape whose scratch would reach 2 GiB are refused.  16-byte    */
/* aligned vectors whose rows are a multiple of 16 bytes take 16-byte   */
/* loads and stores.                                                    */
/* ------------------------------------------------------------------ */

/* bytes of device scratch sa_scr needs for the shape (8-byte aligned, its
 * content is rewritten by every call), or a negative SA_ERR_* code */
int sa_scr_scratch_bytes(uint64_t rows, uint64_t cols, uint64_t inner, int x_type);

int sa_scr(const void* a, const void* b, const void* r, int x_type, uint64_t rows, uint64_t cols, uint64_t inner,
           double threshold, void* sparse_out, void* res_out, void* stats_out, void* scratch, void* stream);

/* ------------------------------------------------------------------ */
/* GaussianModelDP with is_secure_generator (mechanism_fl.py:112-127    */
/* drawing from sfl/security/random/distrbutions.py:89-137): the same   */
/* clip as sa_dp_perturb_f32, the noise from a cryptographic generator  */
/* and combined as Holohan and Braghin describe (arXiv:2107.10138).     */
/* The reference takes its uniforms from the OS CSPRNG; here they are   */
/* a keyed ChaCha20 keystream, so the noise is reproducible from        */
/* (key, nonce, counter) and parallel over the elements.                */
/*                                                                      */
/* Keystream: ChaCha20 as in RFC 8439 section 2.3 (20 rounds, the input */
/* state added at the end).  State words 0-3: the constants 61707865    */
/* 3320646e 79622d32 6b206574; 4-11: the 256-bit key as eight           */
/* little-endian words; 12, 13: the low and high halves of a 64-bit     */
/* block counter B; 14, 15: the low and high halves of a 64-bit nonce.  */
/* (With word 13 read as the RFC's first nonce word this is the RFC's   */
/* layout: its test vector 2.3.2 is B = 0x0900000000000001, nonce       */
/* 0x4a000000.)  The output words are o[0..15].                         */
/*                                                                      */
/* Noise index i = counter0 + e (counter0 % 4 == 0) uses block B = i>>2 */
/* and j = i & 3; a, b, c, d = o[4j .. 4j+3] give two 53-bit uniforms   */
/* (the reference's secrets.randbits(53) / 2**53), all in float64:      */
/*   u1 = (((b << 32) | a) >> 11) * 2^-53                               */
/*   u2 = (((d << 32) | c) >> 11) * 2^-53                               */
/*   r  = sqrt(-2.0 * log(1.0 - u2))      theta = (2.0 * pi) * u1       */
/*   z64 = ((r * sin(theta)) * sigma + (r * cos(theta)) * sigma)        */
/*         / sqrt(2.0)                                                  */
/* in the reference's operation order (u1 drawn first, feeding theta;   */
/* sigma multiplies each Box-Muller output before they are summed);     */
/* 1 - u2 lies in (0, 1], so no draw is infinite.  Then                 */
/*   z32 = (float) z64                    (the reference's astype)      */
/*   x'  = fl32(x * scale) + fl32(z32 / num_updates)                    */
/* with the scale of sa_dp_perturb_f32.  No multiply-add is fused.      */
/* A (key, nonce, counter) triple must never be used twice: the caller  */
/* advances counter0 by whole blocks and draws fresh keys from the OS.  */
/* sa_mask_dp has no secure form (it draws Philox noise): perturb       */
/* first, then sa_mask.                                                 */
/* ------------------------------------------------------------------ */

typedef struct sa_dp_secure {
  const double* sumsq;       /* device: the clipping group's squared norm (sa_sumsq_f32) */
  const double* sumsq_layer; /* device, optional: this layer's squared norm */
  double l2_norm_clip;
  double noise_std;   /* sigma = noise_multiplier * clip * clip, a double */
  float num_updates;  /* divisor of the noise (> 0) */
  uint32_t key[8];    /* ChaCha20 key, little-endian words */
  uint64_t nonce;
  uint64_t counter0;  /* noise index of element 0 (multiple of 4) */
} sa_dp_secure;

/* out = clip-and-secure-noise(x) (out may alias x); 16-byte aligned x and out. */
int sa_dp_perturb_secure_f32(const float* x, uint64_t n, const sa_dp_secure* dp, float* out, void* stream);

/* The raw keystream on the device: out[16 k .. 16 k + 15] = block block0 + k
 * (the block counter wraps mod 2^64), k < n_blocks; out is 16-byte aligned
 * device memory of 16 * n_blocks words. */
int sa_chacha20_keystream(const uint32_t key[8], uint64_t nonce, uint64_t block0, uint64_t n_blocks, uint32_t* out,
                          void* stream);

/* The same blocks on the host (no GPU needed; `out` is host memory): the
 * cipher's known-answer tests.  Not used by any hot-path entry point. */
int sa_chacha20_blocks_host(const uint32_t key[8], uint64_t nonce, uint64_t block0, uint64_t n_blocks,
                            uint32_t* out);

/* The transform alone: out[i] = z64 of the words a, b, c, d = words[4 i ..
 * 4 i + 3] (device memory) -- the function the perturb kernel calls, so
 * its edge inputs (u2 = 0, sin + cos cancelling at u1 = 3/8, 7/8) can be
 * reached, which no search of cipher blocks can. */
int sa_hb_normals_f64(const uint32_t* words, uint64_t n, double sigma, double* out, void* stream);

/* ------------------------------------------------------------------ */
/* COO transport of compressed updates and the sparse server sum: the   */
/* reference's sparse_encode / sparse_decode (sfl/utils/compressor/     */
/* sparse_compressor.py:234-284, wrapping sparse.COO) and the sum of    */
/* its SparsePlainAggregator (sfl/security/aggregation/                 */
/* sparse_plain_aggregator.py:25-139).  A tensor of n elements of       */
/* x_type T (SA_F32 or SA_F64) is (index, data): index the flat         */
/* positions of its non-zeros as int32, strictly ascending, data their  */
/* values bit for bit.  Non-zero is decided on the bit pattern,         */
/* (bits & ~sign) != 0: NaN, inf and every denormal are kept, +0.0 and  */
/* -0.0 are dropped.  n >= 2^31 and other element types are refused.    */
/*   encode: sa_coo_count (pass 1: every wave counts the non-zeros of   */
/*           its contiguous index range; one block turns the counts     */
/*           into exclusive offsets in scratch and writes the total to  */
/*           the device word nnz_out, a uint32), then sa_coo_fill with  */
/*           the same x, n and scratch (pass 2: an entry's rank is its  */
/*           wave's offset plus ballot prefixes; no atomics, no sort).  */
/*           No entry of rank >= cap is stored; a total other than cap  */
/*           sets SA_COO_BAD_COUNT.                                     */
/*   decode: dense_out = 0, then dense_out[index[i]] = data[i].         */
/*   sum:    acc[index[i]] = acc[index[i]] + A(data[i]) * A(w), multiply */
/*           and add rounded separately, for (T, A) = (f32, f32),       */
/*           (f32, f64), (f64, f64); one launch per party on one stream */
/*           (a valid payload's indices are unique: no float atomics,   */
/*           the same bits on every run); then sa_coo_finish,           */
/*           acc[i] = acc[i] / A(divisor).                              */
/* A payload is another party's data.  decode and axpy store entry i    */
/* only if 0 <= index[i] < n -- an index out of range is never used as  */
/* an address -- and report into flag, two uint32 on the device that    */
/* the caller sets to {0, 0xffffffff}: [0] the SA_COO_BAD_* bits met,   */
/* [1] the least offending entry i (an integer atomicMin).  With a bit  */
/* set the content of dense_out / acc is unspecified, but every store   */
/* landed inside it.  Everything is stream-ordered and allocates        */
/* nothing; 16-byte aligned x / acc take 16-byte loads and stores.      */
/* ------------------------------------------------------------------ */
#define SA_COO_BAD_RANGE 1u /* an index outside the tensor */
#define SA_COO_BAD_ORDER 2u /* index[i] <= index[i-1]: unsorted or duplicated */
#define SA_COO_BAD_COUNT 4u /* sa_coo_fill: the number of non-zeros is not cap */

/* bytes of device scratch the encode needs for n elements (4-byte aligned;
 * sa_coo_count writes it, sa_coo_fill reads it), or a negative SA_ERR_* code */
int sa_coo_scratch_bytes(uint64_t n, int x_type);

int sa_coo_count(const void* x, int x_type, uint64_t n, void* scratch, void* nnz_out, void* stream);

int sa_coo_fill(const void* x, int x_type, uint64_t n, const void* scratch, void* index_out, void* data_out,
                uint64_t cap, void* flag, void* stream);

int sa_coo_decode(const void* index, const void* data, int x_type, uint64_t nnz, uint64_t n, void* dense_out,
                  void* flag, void* stream);

int sa_coo_axpy(const void* index, const void* data, int x_type, uint64_t nnz, double w, void* acc, int acc_type,
                uint64_t n, void* flag, void* stream);

int sa_coo_finish(void* acc, int acc_type, uint64_t n, double divisor, void* stream);

/* ------------------------------------------------------------------ */
/* Quantized compressors: the reference's QuantizedZeroPoint,           */
/* QuantizedLSTM and QuantizedFP at 8 bits (sfl/utils/compressor/       */
/* quantized_compressor.py:65-228).  A tensor of n elements of x_type T */
/* (SA_F32 or SA_F64) becomes n codes of q_bytes bytes (1: int8,        */
/* 2: int16) and a few host scalars.  Every operation is rounded in T,  */
/* never fused; `/` is IEEE division, never a multiply by a reciprocal; */
/* rint is round-half-to-even (np.round).  This is the reference's code */
/* as numpy 2 evaluates it (NEP 50: a Python scalar never widens T).    */
/*                                                                      */
/* The scalars are computed on the host between two launches:           */
/*   sa_quant_range   out3 = (min, max, max|x|) of x as three T on the  */
/*           device.  NaN propagates as in np.min / np.max: one NaN     */
/*           anywhere makes all three NaN.  n = 0 gives (inf, -inf, 0). */
/*           The sign of a zero result is unspecified.  Two stages:     */
/*           every block reduces its share to one partial in scratch,   */
/*           one block reduces the partials; no atomics, so the same    */
/*           input gives the same bits on every run.                    */
/*   zero point (mode SA_QUANT_ZERO_POINT; p0 = scale, p1 = z), for     */
/*           qmin = -2^(bits-1), qmax = 2^(bits-1) - 1:                 */
/*             scale = T(max - min) / T(qmax - qmin)                    */
/*             z     = qmin - T(min / scale), clamped to [qmin, qmax],  */
/*                     truncated to an integer                          */
/*             code  = int(rint(min(max(x / scale + T(z), qmin), qmax))) */
/*             dec   = (T(code) - T(z)) * scale                         */
/*   LSTM (mode SA_QUANT_LSTM; p0 = q, p1 = T(rqm)):                    */
/*             q     = T(2^bits - 1) / T(max - min)                     */
/*             rqm   = int(rint(T(q * min))) + 2^(bits-1)               */
/*             code  = int(min(max(rint(q * x) - T(rqm), qmin), qmax))  */
/*             dec   = (T(code) + T(rqm)) / q                           */
/*           with [qmin, qmax] the storage range of the codes.  The     */
/*           clamp is a refinement: the reference casts without it, and */
/*           an out-of-range float-to-int8 cast wraps on x86, turning   */
/*           the largest element into the smallest.                     */
/*   fp8 (mant_len, exp_offset) = (8, 6) for E4M3 with max_value 448,   */
/*           (4, 14) for E5M2 with max_value 57344:                     */
/*             scale = T(max_value) / (max|x| > 0 ? max|x| : 1)         */
/*             m, e  = frexp(|x| * scale)                               */
/*             qe    = e > -exp_offset ? e + exp_offset : 0             */
/*             qm    = rint((2 m - 1) * mant_len); qm = mant_len is a   */
/*                     carry into the exponent field, as intended       */
/*             code  = sign(x) * (qe * mant_len + qm)       (an int8)   */
/*             c     = |code| as an int32, so -128 is 128 (numpy's int8 */
/*                     abs wraps: the second refinement; the encoder    */
/*                     never emits -128)                                */
/*             dec   = sign(code) * ldexp(((c % mant_len) / T(mant_len) */
/*                     + 1) / 2, c / mant_len - exp_offset) / scale     */
/*           A scaled magnitude below 2^-exp_offset gets qe = 0 and     */
/*           keeps its mantissa field only, as in the reference: it     */
/*           decodes into [2^-(exp_offset+1), 2^-exp_offset) / scale,   */
/*           or to 0 when that field is 0; x = 0 gives code 0.          */
/* p0, p1 and scale are doubles that carry T values exactly.  The       */
/* kernels do not validate the scalars: the callers refuse a range that */
/* is not finite (sfl_amd/utils/quantized.py), and x outside what the   */
/* scalars were computed for gives saturated or unspecified codes, but  */
/* every store lands inside q_out / out.                                */
/* A lane packs the codes of consecutive elements in registers and      */
/* stores at least 4 bytes at once; a scalar head of fewer than 16      */
/* elements aligns the codes for that store, a scalar tail takes what   */
/* is left of the last run.  The float vector takes 16-byte accesses if */
/* it is 16-byte aligned behind the head.  Every vector is element-     */
/* aligned; nothing may alias.  n >= 2^32, other element types, q_bytes */
/* other than 1 or 2, an unknown mode or fp8 format and a clamp range   */
/* outside the storage type are refused before any launch.  Everything  */
/* is stream-ordered and allocates nothing.                             */
/* ------------------------------------------------------------------ */
#define SA_QUANT_ZERO_POINT 0
#define SA_QUANT_LSTM 1

/* bytes of device scratch sa_quant_range needs for n elements (8-byte
 * aligned, rewritten by every call), or a negative SA_ERR_* code */
int sa_quant_scratch_bytes(uint64_t n, int x_type);

int sa_quant_range(const void* x, int x_type, uint64_t n, void* scratch, void* out3, void* stream);

int sa_quant_affine(const void* x, int x_type, uint64_t n, int mode, double p0, double p1, int qmin, int qmax,
                    void* q_out, int q_bytes, void* stream);

int sa_dequant_affine(const void* q, int q_bytes, uint64_t n, int mode, double p0, double p1, int x_type, void* out,
                      void* stream);

int sa_quant_fp8(const void* x, int x_type, uint64_t n, double scale, int mant_len, int exp_offset, void* q_out,
                 void* stream);

int sa_dequant_fp8(const void* q, uint64_t n, double scale, int mant_len, int exp_offset, int x_type, void* out,
                   void* stream);

/* data_out[i] = x[index[i]], i < nnz: a tensor's values at a mask's
 * positions, zeros included.  The mask is validated like a payload: an index
 * outside [0, n) is never used as an address and sets SA_COO_BAD_RANGE, one
 * not above its predecessor SA_COO_BAD_ORDER, flag[1] the least such i; the
 * entries of data_out behind a flagged index are unspecified.  data_out may
 * alias nothing. */
int sa_coo_gather(const void* index, uint64_t nnz, const void* x, int x_type, uint64_t n, void* data_out, void* flag,
                  void* stream);

/* ------------------------------------------------------------------ */
/* Top-k sparsification: the reference's TopkSparse and RandomSparse    */
/* (sfl/utils/compressor/sparse_compressor.py:97-139).  Of n keys of    */
/* key_type (SA_F32 or SA_F64) the k of largest magnitude are kept,     */
/* ordered by the bit pattern of |key| as an unsigned integer (numpy's  */
/* order, NaN last, so NaN is kept first).  Equal keys at the           */
/* threshold: the HIGHER indices are kept, so the kept set is the       */
/* complement of what sa_stc masks at mask_num = n - k.  The payload is */
/* (index, data) as in the COO block: the kept flat positions as int32, */
/* strictly ascending, and x at those positions, bit for bit.           */
/*   sa_topk_select: sa_stc's radix select over keys for rank           */
/*           n - k - 1 (one histogram pass and one one-block scan per   */
/*           digit: 3 digits for float32, 6 for float64), one counting  */
/*           pass (per wave: the keys above the threshold and the ties  */
/*           at it) and one block that turns the tie counts into each   */
/*           wave's first tie rank and the kept counts into exclusive   */
/*           output offsets, all in scratch.  k == 0 and k == n skip    */
/*           the digit passes.                                          */
/*   sa_topk_fill: with the same keys, n, k and scratch, every wave     */
/*           re-reads its range and stores index_out[rank] = e,         */
/*           data_out[rank] = x[e]; ranks come from ballot prefixes     */
/*           (no atomics, no sort).  x may be keys itself (one load) or */
/*           another vector of n elements of x_type.  No entry of rank  */
/*           >= k is stored; a total other than k (keys changed between */
/*           the two calls) sets SA_COO_BAD_COUNT in flag, the two-word */
/*           record of the COO entries.  index_out and data_out may     */
/*           alias nothing.                                             */
/*   sa_topk_random_keys: RandomSparse's keys, n 8-byte words.  Element */
/*           e takes words w[2e], w[2e+1] of the Philox4x32-10 stream   */
/*           under the 64-bit seed (counter block e >> 1 = (lo, hi, 0,  */
/*           0), key words (seed lo, seed hi); words 0, 1 for even e,   */
/*           2, 3 for odd e): key = ((w[2e+1] << 32) | w[2e]) >> 1, 63  */
/*           bits.  Read as float64 bit patterns (key_type SA_F64) by   */
/*           the two entries above, the k largest keys are k positions  */
/*           drawn uniformly without replacement.                       */
/*           sa_topk_random_keys_host: the same words in host memory,   */
/*           no GPU needed.                                             */
/* n >= 2^31, other element types and k > n are refused before any      */
/* launch; n == 0 returns before the pointers are looked at.            */
/* Everything is stream-ordered, allocates nothing, uses no float       */
/* atomics and never synchronises with the host; the same input gives   */
/* the same bits on every run.  16-byte aligned vectors take 16-byte    */
/* loads.                                                               */
/* ------------------------------------------------------------------ */

/* bytes of device scratch the two entries share for n keys (8-byte aligned;
 * sa_topk_select writes it, sa_topk_fill reads it), or a negative SA_ERR_* code */
int sa_topk_scratch_bytes(uint64_t n, int key_type);

int sa_topk_select(const void* keys, int key_type, uint64_t n, uint64_t k, void* scratch, void* stream);

int sa_topk_fill(const void* keys, int key_type, const void* x, int x_type, uint64_t n, uint64_t k,
                 const void* scratch, void* index_out, void* data_out, void* flag, void* stream);

int sa_topk_random_keys(uint64_t seed, uint64_t n, void* keys_out, void* stream);

int sa_topk_random_keys_host(uint64_t seed, uint64_t n, void* keys_out);

/* ------------------------------------------------------------------ */
/* QuantizedKmeans: the reference's class (sfl/utils/compressor/        */
/* quantized_compressor.py:231-279) with the fit pinned, a 1-D k-means  */
/* run in integers (sfl_amd/utils/quantized.py has the definition).     */
/* A tensor of n elements of x_type T (SA_F32 or SA_F64), n < 2^32, is  */
/* seen through its 32-bit image                                        */
/*   u = min(2^32 - 1, uint64(rint((double(x) - mn) * s)))              */
/* with host scalars mn and s = (2^32 - 1) / (mx - mn); the subtraction */
/* and the multiplication round separately, never fused.  Every entry   */
/* computes the image anew; nothing of it is stored.                    */
/*   sa_kmeans_hist    hist[b] = the number of u with u >> 20 == b,     */
/*           SA_KMEANS_BINS uint32 on the device (zeroed by the call):  */
/*           what the host forms the start from                         */
/*           (quantized_compressor.py:231-279 starts at random).        */
/*   sa_kmeans_step    `steps` Lloyd steps on the state block, enqueued */
/*           back to back (quantized_compressor.py:231-279: the fit).   */
/*           The state, SA_KMEANS_STATE_BYTES on the device, 8-byte     */
/*           aligned, written by the caller before the first step:      */
/*             uint64 sum[256]; uint32 cnt[256]; uint32 c[256];         */
/*             uint32 done, n_iter;                                     */
/*           all zero but the k sorted centres c[0 .. k-1]              */
/*           (SA_KMEANS_STATE_C bytes in; done at SA_KMEANS_STATE_DONE, */
/*           n_iter behind it).  A step: b_j = (c_j + c_{j+1}) >> 1;    */
/*           label(u) = the number of j with b_j < u; cnt_j and sum_j   */
/*           over the labels; c'_j = sum_j / cnt_j rounded half up, an  */
/*           empty cluster keeps c_j; n_iter += 1; done = 1 if no       */
/*           centre moved.  A step that finds done set does nothing.    */
/*           Counts and sums are integers added with integer atomics:   */
/*           order-free, so the same input gives the same bits.         */
/*   sa_kmeans_labels  q_out[i] = label(u_i) - offset under the state's */
/*           centres, as q_bytes-byte codes (1: int8, 2: int16) in      */
/*           sa_quant_affine's layout (quantized_compressor.py:231-279: */
/*           labels_ - 2^(quant_bits-1)).                               */
/*   sa_dequant_lut    out[i] = lut[q[i] + offset], lut k values of T   */
/*           on the device, in sa_dequant_affine's layout               */
/*           (quantized_compressor.py:231-279: _decompress_one).  The   */
/*           codes are another party's data: one whose label is outside */
/*           [0, k) is never used as an index, gives 0 and reports into */
/*           flag, two uint32 the caller sets to {0, 0xffffffff}:       */
/*           [0] |= SA_KMEANS_BAD_CODE, [1] the least such i.           */
/* Other element types, n >= 2^32, k outside 2 .. SA_KMEANS_MAX_K, an   */
/* offset that lets a code leave its storage type and misaligned        */
/* pointers are refused before any launch.  x outside [mn, mx] images   */
/* to 0 or 2^32 - 1; every store lands inside its output.  Everything   */
/* is stream-ordered, allocates nothing, uses no float atomics and      */
/* never synchronises with the host.                                    */
/* ------------------------------------------------------------------ */
#define SA_KMEANS_MAX_K 256
#define SA_KMEANS_BINS 4096
#define SA_KMEANS_STATE_BYTES 4104
#define SA_KMEANS_STATE_C 3072
#define SA_KMEANS_STATE_DONE 4096
#define SA_KMEANS_BAD_CODE 1u /* a code whose label is outside [0, k) */

/* bytes of device scratch a fit needs for n elements: the histogram, then the
 * state block (8-byte aligned), or a negative SA_ERR_* code */
int sa_kmeans_scratch_bytes(uint64_t n, int x_type);

int sa_kmeans_hist(const void* x, int x_type, uint64_t n, double mn, double s, void* hist, void* stream);

int sa_kmeans_step(const void* x, int x_type, uint64_t n, double mn, double s, int k, int steps, void* state,
                   void* stream);

int sa_kmeans_labels(const void* x, int x_type, uint64_t n, double mn, double s, int k, const void* state, int offset,
                     void* q_out, int q_bytes, void* stream);

int sa_dequant_lut(const void* q, int q_bytes, uint64_t n, const void* lut, int k, int offset, int x_type, void* out,
                   void* flag, void* stream);

/* ------------------------------------------------------------------ */
/* FlameAggregator: the per-element work of the reference's robust      */
/* aggregator (examples/security/h_bd/agg_flame.py:27-203) for C        */
/* clients, 1 <= C <= SA_FLAME_MAX_CLIENTS, whose tensors of n elements */
/* of x_type T (SA_F32 or SA_F64), n < 2^32, live on one device.  x is  */
/* a HOST table of C device pointers; it reaches the kernels by value.  */
/* The definition (sfl_amd/security/aggregation/flame_aggregator.py has */
/* the host form and the decisions between the two entries):            */
/*   median  g = the median of the C values of an element, in T: the    */
/*           middle one for odd C, (lo + hi) / T(2) for even C with the */
/*           add and the divide each rounded in T (the add may overflow */
/*           to inf, as numpy's); a NaN among the C gives NaN.  Order:  */
/*           the total order of the bit patterns, -0 < +0.              */
/*   stats   C (C + 1) / 2 + C float64:                                 */
/*             G[i][j] = sum x_i x_j, i <= j, operands converted to     */
/*                       float64 first, at [i C - i (i - 1) / 2 + j - i]*/
/*                       (the packed upper triangle, row-major)         */
/*             N[i]    = sum d_i^2, d_i = x_i - g rounded in T, squared */
/*                       in float64, at [C (C + 1) / 2 + i]             */
/*           The order of summation is fixed: a lane's tiles in index   */
/*           order, a wave's lanes by one butterfly, a block's waves in */
/*           wave order, the blocks in block order by one block; the    */
/*           grid is a function of n only.  No atomics: the same input  */
/*           gives the same bits on every run.                          */
/*   sa_flame_stats    writes g into median_out (n elements of T) and   */
/*           this tensor's stats into `stats` (device): added to what   */
/*           is there when `accumulate`, else stored (agg_flame.py:     */
/*           61-73 the median, :79-89 and :128-132 the update norms,    */
/*           :95-112 the cosine distances' Gram matrix).  Layers are    */
/*           added in call order.  scratch: sa_flame_scratch_bytes      */
/*           bytes on the device, 8-byte aligned, rewritten by every    */
/*           call.  n == 0 looks at no pointer but stats and stores     */
/*           zeros (or adds nothing).  Up to 8 clients one pass over    */
/*           the tensors; above, two (the Gram matrix's rows split).    */
/*   sa_flame_combine  out[e] = (sum over the kept clients, in order,   */
/*           of float64(g + (x_i - g) T(scale_i)) weight_i) / divisor   */
/*           + 0.0, n float64 on the device (agg_flame.py:141-168 the   */
/*           clipping, :181-187 np.average, :193-199 the zero-variance  */
/*           noise term).  The inner expression rounds in T after every */
/*           operation, the outer multiply and add round separately,    */
/*           nothing is contracted; the sum starts from +0.0.  scale    */
/*           and weight are HOST arrays of C doubles.  A client whose   */
/*           weight is a NaN is dropped: its pointer is not looked at   */
/*           and its tensor never read.  At least one client is kept.   */
/* Other element types, n >= 2^32, a client count outside 1 ..          */
/* SA_FLAME_MAX_CLIENTS, null and misaligned pointers are refused       */
/* before any launch.  16-byte aligned vectors take 16-byte accesses;   */
/* others element accesses with the same lane-to-element map.  Nothing  */
/* may alias an output.  Everything is stream-ordered, allocates        */
/* nothing and never synchronises with the host.                        */
/* ------------------------------------------------------------------ */
#define SA_FLAME_MAX_CLIENTS 16

/* bytes of device scratch sa_flame_stats needs for n elements of n_clients
 * clients (the blocks' partial sums), or a negative SA_ERR_* code */
int sa_flame_scratch_bytes(uint64_t n, int n_clients, int x_type);

int sa_flame_stats(const void* const* x, int n_clients, int x_type, uint64_t n, void* median_out, void* scratch,
                   double* stats, int accumulate, void* stream);

int sa_flame_combine(const void* const* x, const double* scale, const double* weight, int n_clients, int x_type,
                     uint64_t n, const void* median, double divisor, double* out, void* stream);

/* ------------------------------------------------------------------ */
/* FedSMP: sparsified model perturbation (examples/security/h_gia/      */
/* FedSMP_defense/FedSMP_torch.py:105-119 the worker, :193-201 the      */
/* server's mask).  A worker uploads                                    */
/*   w0 + mask * GaussianModelDP(mask * (w1 - w0) / (p + 1e-6))         */
/* for the round's weights w0, its trained weights w1 and a random 0/1  */
/* mask of keep ratio p.  Here (sfl_amd/security/privacy/smp.py has the */
/* host form):                                                          */
/*   mask    keyed, never shipped: element e of a layer has stream      */
/*           index i = counter0 + e (counter0 % 4 == 0: the sum of      */
/*           ceil(n / 4) * 4 over the float32 layers before it, the     */
/*           layout of sa_dp's counter0); w_i = word i & 3 of           */
/*           Philox4x32-10 on the counter block (lo32(i >> 2),          */
/*           hi32(i >> 2), 1, 0) under the key words (lo32(key),        */
/*           hi32(key)); the element is KEPT iff w_i < threshold,       */
/*           compared in 64 bits, threshold = min(2^32, int(p * 2^32)): */
/*           2^32 keeps everything, 0 nothing.  The 1 in the third      */
/*           counter word keeps the mask's words apart from the DP      */
/*           noise's (0 there) under one key.                           */
/*   d       = kept ? (w1 - w0) / divisor : +0, float32, the subtract   */
/*           and the IEEE division each rounded once; divisor =         */
/*           np.float32(p + 1e-6), the double sum rounded once.         */
/*   norm    a layer's squared norm is sa_sumsq_f32's definition        */
/*           applied to d: sa_smp_sumsq_f32 is bit for bit sa_sumsq_f32 */
/*           of sa_smp_delta_f32's output (the same grid, lane map,     */
/*           order of additions and final step; one body, two loaders). */
/*   t       = d * scale + (z * sigma) / num_updates, sa_dp_perturb_f32 */
/*           on d: z the normal of noise index dp->counter0 + e; the    */
/*           normals of dropped elements are skipped, never reused.     */
/*   out     = kept ? w0 + t : w0 (a dropped element has w0's bits);    */
/*           without a dp, kept ? w0 + d : w0.                          */
/* Differences from the reference, on purpose: float32 throughout (its  */
/* int64 mask promotes the update, the norm and the upload to float64); */
/* a select where it multiplies by 0 (0 * inf is NaN there, and a zero  */
/* weight can change sign); the mask from (key, p) instead of an int64  */
/* array from numpy's unseeded global stream (parity for the mask is    */
/* distributional, as for the noise).                                   */
/* float32 vectors are 16-byte aligned; n == 0 returns before they are  */
/* looked at.  counter0 % 4 != 0, threshold > 2^32, a divisor that is   */
/* not positive (where the entry divides), null or misaligned vectors   */
/* and an n beyond the tile grid are refused before any launch.         */
/* Everything is stream-ordered, allocates nothing, uses no atomics and */
/* gives the same bits on every run.  ABI version 3 (additive).         */
/* ------------------------------------------------------------------ */
typedef struct sa_smp {
  uint64_t key;       /* Philox key of the round's mask */
  uint64_t counter0;  /* stream index of element 0 (multiple of 4) */
  uint64_t threshold; /* kept iff word < threshold; at most 2^32 */
  float divisor;      /* np.float32(p + 1e-6) */
} sa_smp;

/* out[e] = 1 if element e is kept, else 0: n bytes of host memory (no GPU needed) */
int sa_smp_mask_host(const sa_smp* smp, uint64_t n, uint8_t* out);

/* the same bytes on the device */
int sa_smp_mask(const sa_smp* smp, uint64_t n, uint8_t* out, void* stream);

/* out = d, materialised (out may alias w1) */
int sa_smp_delta_f32(const float* w0, const float* w1, uint64_t n, const sa_smp* smp, float* out, void* stream);

/* *sumsq (+)= the squared norm of d as sa_sumsq_f32 forms it, d never stored;
 * `partials` is caller scratch of SA_DP_PARTIALS doubles */
int sa_smp_sumsq_f32(const float* w0, const float* w1, uint64_t n, const sa_smp* smp, double* partials,
                     double* sumsq, int accumulate, void* stream);

/* the upload in one pass: out = kept ? w0 + t : w0; dp may be NULL (t = d);
 * out may alias w1 */
int sa_smp_perturb_f32(const float* w0, const float* w1, uint64_t n, const sa_smp* smp, const sa_dp* dp, float* out,
                       void* stream);

/* out = kept ? w0 + t : w0 for a t formed elsewhere (sa_smp_delta_f32, then
 * any model-level DP): the last step of the unfused path; out may alias t */
int sa_smp_finish_f32(const float* w0, const float* t, uint64_t n, const sa_smp* smp, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SFL_SA_H */
