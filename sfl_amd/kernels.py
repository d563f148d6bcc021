"""Tensor-level wrappers of the HIP hot path (libsfl_sa.so via ctypes).

PyTorch is plumbing here: it owns device memory and streams; the work is done
by the hand-written gfx950 kernels behind the C-ABI.  uint64 buffers are
carried as ``torch.int64`` tensors (same bits); ``as_u64`` gives numpy views.

Every function launches asynchronously on the current torch stream of the
tensors' device and raises ``SALibraryError`` on any error.  Nothing here
falls back to a CPU implementation.
"""

from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from . import _lib as L

U64 = torch.int64  # storage dtype for uint64 buffers

_XTYPE = {torch.float32: L.SA_F32, torch.float64: L.SA_F64, torch.int64: L.SA_I64}


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t: torch.Tensor) -> int:
    """The current torch stream of ``t``'s device, as the raw handle the C-ABI
    takes (torch's raw-stream binding costs ~1 us where
    ``torch.cuda.current_stream(device)`` costs ~5 us: small calls launch
    several kernels, tools/latency_profile.py)."""
    if _raw_stream is not None:
        return _raw_stream(t.device.index)
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _require_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("libsfl_sa kernels take device-resident tensors")


def as_u64(t: torch.Tensor) -> np.ndarray:
    """Host numpy uint64 view of a uint64-carrying int64 tensor: a device
    tensor is read through a pinned buffer (``hostpipe.d2h``, no pageable
    DMA), a CPU tensor is viewed in place."""
    if t.device.type == "cpu":
        return t.detach().numpy().view(np.uint64)
    from . import hostpipe as H

    return H.d2h(t, pooled=False).view(np.uint64)


def xtype_of(dtype: torch.dtype) -> int:
    try:
        return _XTYPE[dtype]
    except KeyError:
        raise TypeError(f"unsupported element type {dtype}; use float32, float64 or int64") from None


def make_streams(entries: Sequence[tuple]) -> C.Array:
    """entries: (L.PCG64 gen, sign, peer) -> sa_mask_stream[]"""
    arr = (L.MaskStream * max(1, len(entries)))()
    for i, (g, sign, peer) in enumerate(entries):
        arr[i].gen = g
        arr[i].sign = int(sign)
        arr[i].peer = int(peer)
    return arr


def _pair_arrays(n_clients: int, pair_gens: Sequence, pair_signs: Sequence[int]) -> tuple[C.Array, C.Array]:
    """sa_pcg64[] / int8[] of the n_clients * (n_clients - 1) / 2 internal pairs (never empty arrays)"""
    npair = n_clients * (n_clients - 1) // 2
    return (L.PCG64 * max(1, npair))(*pair_gens), (C.c_int8 * max(1, npair))(*[int(s) for s in pair_signs])


def mask(x: torch.Tensor | None, out: torch.Tensor, streams: Sequence[tuple], *,
         weight: float = 1.0, weight_vec: torch.Tensor | None = None, compute_dtype=None,
         fxp_bits: int = 18, x_dtype=None, sum_accum: torch.Tensor | None = None,
         digest: torch.Tensor | None = None, flags: torch.Tensor | None = None) -> torch.Tensor:
    """One client's masked vector: out = trunc(x*w*2^fxp) +/- masks (mod 2^64).
    ``x=None`` continues from ``out`` (multi-pass).  See sa_mask in include/sfl_sa.h."""
    _require_gpu(x, out, weight_vec, sum_accum, digest, flags)
    n = out.numel()
    if x is not None and x.numel() != n:
        raise ValueError("x and out sizes differ")
    xt = xtype_of(x.dtype if x is not None else (x_dtype or torch.float32))
    ct = xtype_of(compute_dtype) if compute_dtype is not None else xt
    sarr = make_streams(streams)
    L.check(L.lib().sa_mask(_ptr(x), xt, ct, n, float(weight), _ptr(weight_vec), int(fxp_bits),
                            sarr, len(streams), _ptr(out), _ptr(sum_accum), _ptr(digest),
                            _ptr(flags), C.c_void_p(_stream(out))), "sa_mask")
    return out


def fused_clients(xs: Sequence[torch.Tensor], weights: Sequence[float], pair_gens: Sequence,
                  pair_signs: Sequence[int], cross: Sequence[tuple], n_cross: int,
                  sum_out: torch.Tensor, *, fxp_bits: int = 18, accumulate: bool = False,
                  digests: torch.Tensor | None = None, flags: torch.Tensor | None = None,
                  masked_outs: Sequence[torch.Tensor | None] | None = None) -> torch.Tensor:
    """C co-located clients in one launch: quantize, pairwise masks, masked sum.
    See sa_fused_clients in include/sfl_sa.h."""
    _require_gpu(sum_out, digests, flags, *xs)
    nc = len(xs)
    n = sum_out.numel()
    clients = (L.LocalClient * nc)()
    for c, x in enumerate(xs):
        if x.numel() != n or x.dtype != xs[0].dtype:
            raise ValueError("fused clients need equal-size vectors of one dtype")
        clients[c].x = x.data_ptr()
        clients[c].weight = float(weights[c])
        mo = masked_outs[c] if masked_outs else None
        clients[c].masked_out = mo.data_ptr() if mo is not None else None
    pg, ps = _pair_arrays(nc, pair_gens, pair_signs)
    carr = make_streams(cross)
    rc = L.lib().sa_fused_clients(clients, nc, xtype_of(xs[0].dtype), n, int(fxp_bits), pg, ps,
                                  carr, int(n_cross), _ptr(sum_out), int(bool(accumulate)),
                                  _ptr(digests), _ptr(flags), C.c_void_p(_stream(sum_out)))
    if rc == L.SA_ERR_UNSUPPORTED:
        if (nc > 8 and n_cross == 0 and digests is None and not (masked_outs and any(m is not None for m in masked_outs))
                and xs[0].dtype == torch.float32):
            # more co-located clients than one launch holds, only the sum wanted:
            # the pair-shared schedule (every pair stream still expanded once)
            return fused_many(xs, weights, pair_gens, pair_signs, sum_out, fxp_bits=fxp_bits,
                              accumulate=accumulate, flags=flags)
        # other shapes without a fused instantiation (e.g. 32 clients, 4 per
        # GPU, with cross streams; or per-client digests / wire images): every
        # client masks with its own streams (both ends of each internal pair)
        # and accumulates into the sum -- same result, no pair sharing
        return _fused_fallback(xs, weights, pair_gens, pair_signs, cross, n_cross, sum_out, fxp_bits,
                               accumulate, digests, flags, masked_outs)
    L.check(rc, "sa_fused_clients")
    return sum_out


def many_schedule(nc: int) -> tuple[list[list[int]], list[tuple[list[int], list[int]]]]:
    """The pair-shared schedule of ``nc`` co-located clients (more than one
    launch holds): clients in quads of 4 (the last may be short), quads in
    groups of two.  Returns (groups, bipartite blocks): one sa_fused_clients
    launch per group (its clients' quantized values and every pair inside the
    group) and one sa_fused_bipartite launch per pair of quads in different
    groups (their cross pairs) -- every pair of clients exactly once."""
    quads = [list(range(q, min(nc, q + 4))) for q in range(0, nc, 4)]
    groups = [quads[g] + (quads[g + 1] if g + 1 < len(quads) else []) for g in range(0, len(quads), 2)]
    blocks = [(quads[a], quads[b]) for a in range(len(quads)) for b in range(a + 1, len(quads)) if a // 2 != b // 2]
    return groups, blocks


_PAD_STREAM = (0, 1)  # (state, inc) of a padding slot's pairs: drawn, and cancelled in the sum


def fused_many(xs: Sequence[torch.Tensor], weights: Sequence[float], pair_gens: Sequence, pair_signs: Sequence[int],
               sum_out: torch.Tensor, *, fxp_bits: int = 18, accumulate: bool = False,
               flags: torch.Tensor | None = None) -> torch.Tensor:
    """Masked sum of ``len(xs)`` co-located float32 clients (any number) with
    every pair stream expanded ONCE and applied to both of its clients
    (``many_schedule``; ``pair_gens`` / ``pair_signs`` in sa_fused_clients'
    u-major order).  All launches add into ``sum_out``; the sum equals the
    per-client path's bit for bit.  A short last quad is padded with slots
    that have no input and dummy pair streams, whose masks cancel in the sum."""
    _require_gpu(sum_out, flags, *xs)
    nc, n = len(xs), sum_out.numel()
    pidx, p = {}, 0
    for u in range(nc):
        for v in range(u + 1, nc):
            pidx[(u, v)] = p
            p += 1
    groups, blocks = many_schedule(nc)
    first = not accumulate
    for grp in groups:
        gp = [(u, v) for i, u in enumerate(grp) for v in grp[i + 1:]]
        fused_clients([xs[c] for c in grp], [weights[c] for c in grp], [pair_gens[pidx[q]] for q in gp],
                      [pair_signs[pidx[q]] for q in gp], [], 0, sum_out, fxp_bits=fxp_bits, accumulate=not first,
                      flags=flags)
        first = False
    pad = L.PCG64.of(*_PAD_STREAM)
    clients = (L.LocalClient * 8)()
    for c in range(8):
        clients[c].x, clients[c].weight, clients[c].masked_out = None, 1.0, None
    for qa, qb in blocks:
        gens, signs = [], []
        for i in range(4):
            for j in range(4):
                if i < len(qa) and j < len(qb):
                    q = pidx[(qa[i], qb[j])]
                    gens.append(pair_gens[q])
                    signs.append(int(pair_signs[q]))
                else:
                    gens.append(pad)
                    signs.append(1)
        L.check(L.lib().sa_fused_bipartite(clients, L.SA_F32, n, int(fxp_bits), (L.PCG64 * 16)(*gens),
                                           (C.c_int8 * 16)(*signs), _ptr(sum_out), 1, _ptr(flags),
                                           C.c_void_p(_stream(sum_out))), "sa_fused_bipartite")
    return sum_out


def _fused_fallback(xs, weights, pair_gens, pair_signs, cross, n_cross, sum_out, fxp_bits, accumulate,
                    digests, flags, masked_outs):
    nc = len(xs)
    per = [[] for _ in range(nc)]
    p = 0
    for u in range(nc):
        for v in range(u + 1, nc):
            per[u].append((pair_gens[p], int(pair_signs[p]), v))
            per[v].append((pair_gens[p], -int(pair_signs[p]), u))
            p += 1
    for c in range(nc):
        per[c].extend(cross[c * n_cross:(c + 1) * n_cross])
    if not accumulate:
        sum_out.zero_()
    scratch = None
    for c in range(nc):
        out = masked_outs[c] if masked_outs and masked_outs[c] is not None else None
        if out is None:
            scratch = scratch if scratch is not None else torch.empty_like(sum_out)
            out = scratch
        mask(xs[c], out, per[c], weight=weights[c], fxp_bits=fxp_bits, sum_accum=sum_out,
             digest=None if digests is None else digests[c:c + 1], flags=flags)
    return sum_out


def sum_u64(ins: Sequence[torch.Tensor], out: torch.Tensor) -> torch.Tensor:
    """Server sum mod 2^64 of masked vectors."""
    _require_gpu(out, *ins)
    n = out.numel()
    for t in ins:
        if t.numel() != n or t.device != out.device:
            raise ValueError("sum_u64 inputs must match out in size and device")
    ptrs = (C.c_void_p * len(ins))(*[t.data_ptr() for t in ins])
    L.check(L.lib().sa_sum_u64(ptrs, len(ins), n, _ptr(out), C.c_void_p(_stream(out))), "sa_sum_u64")
    return out


def decode(s: torch.Tensor, out: torch.Tensor, *, fxp_bits: int = 18, divisor: float = 1.0,
           divisor_vec: torch.Tensor | None = None) -> torch.Tensor:
    """float64 out = (int64)s / 2^fxp / divisor (or / divisor_vec[i])."""
    _require_gpu(s, out, divisor_vec)
    L.check(L.lib().sa_decode(_ptr(s), s.numel(), int(fxp_bits), float(divisor), _ptr(divisor_vec),
                              _ptr(out), C.c_void_p(_stream(out))), "sa_decode")
    return out


def _scratch(pinned: torch.Tensor, dev: torch.Tensor, need_pin: int, need_dev: int) -> None:
    _require_gpu(dev)
    if not pinned.is_pinned() or pinned.numel() < need_pin or dev.numel() < need_dev:
        raise ValueError("scratch buffers too small or not page-locked")


def _pad_meta(n: int, meta_words: int) -> tuple[int, int]:
    """(n_pad, meta words rounded to even) of csrc/sa_host_layout.h, which tests/test_boundary.py holds the
    four ``*_scratch`` below equal to; not asked of the library: a small call counts microseconds (``_stream``)."""
    return -(-n // 4) * 4, (meta_words + 1) // 2 * 2


def host_fused_scratch(n_clients: int, n: int) -> tuple[int, int]:
    """(pinned bytes, device bytes) sa_fused_clients_host_f32 needs."""
    n_pad, meta = _pad_meta(n, 1 + n_clients)  # flag + digests
    pin = n_clients * n_pad * 4 + (meta + n_pad) * 8
    return pin, pin + n_pad * 8


def fused_clients_host_f32(xs: Sequence[np.ndarray], weights: Sequence[float], pair_gens: Sequence,
                           pair_signs: Sequence[int], pinned: torch.Tensor, dev: torch.Tensor, *,
                           fxp_bits: int = 18, divisor: float = 1.0):
    """Host float32 vectors of 2..8 co-located clients -> (decoded float64
    host array, uint64 digests, flag word) in ONE blocking call (see
    sa_fused_clients_host_f32 in include/sfl_sa.h).  ``pinned`` / ``dev``:
    byte tensors of host_fused_scratch's sizes (page-locked / on the GPU).
    None when the library has no fused kernel for this client count."""
    nc, n = len(xs), int(xs[0].size)
    _scratch(pinned, dev, *host_fused_scratch(nc, n))
    arrs = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in xs]
    if any(a.size != n for a in arrs):
        raise ValueError("fused clients need equal-size vectors")
    ptrs = (C.c_void_p * nc)(*[a.ctypes.data for a in arrs])
    ws = (C.c_double * nc)(*[float(w) for w in weights])
    pg, ps = _pair_arrays(nc, pair_gens, pair_signs)
    out = np.empty(n, dtype=np.float64)
    digests = np.empty(nc, dtype=np.uint64)
    flags = C.c_uint32(0)
    rc = L.lib().sa_fused_clients_host_f32(ptrs, ws, nc, n, int(fxp_bits), pg, ps, float(divisor),
                                           _ptr(pinned), _ptr(dev), C.c_void_p(out.ctypes.data),
                                           C.c_void_p(digests.ctypes.data), C.byref(flags),
                                           C.c_void_p(_stream(dev)))
    if rc == L.SA_ERR_UNSUPPORTED:
        return None
    L.check(rc, "sa_fused_clients_host_f32")
    return out, digests, int(flags.value)


_NP_XTYPE = {np.dtype(np.float32): L.SA_F32, np.dtype(np.float64): L.SA_F64, np.dtype(np.int64): L.SA_I64}


def host_clients_scratch(n_clients: int, n: int, itemsize: int) -> tuple[int, int]:
    """(pinned bytes, device bytes) sa_clients_host needs."""
    n_pad, meta = _pad_meta(n, 1 + n_clients)
    pin = n_clients * n_pad * itemsize + (2 * n_pad + meta) * 8
    return pin, pin + n_clients * n_pad * 8


def clients_host(xs: Sequence[np.ndarray], compute_dtype, weights: Sequence[float], streams: Sequence[Sequence],
                 pinned: torch.Tensor, dev: torch.Tensor, *, fxp_bits: int = 18, divisor: float = 1.0):
    """Host vectors of one element type (float32 / float64 / int64) of 2..9
    co-located clients, each masked with its own streams (``streams[c]``:
    (gen, sign, peer) triples) -> (decoded float64 host array, uint64
    digests, flag word) in ONE blocking call (sa_clients_host in
    include/sfl_sa.h)."""
    nc, n = len(xs), int(np.asarray(xs[0]).size)
    dt = np.asarray(xs[0]).dtype
    arrs = [np.ascontiguousarray(x, dtype=dt).reshape(-1) for x in xs]
    if dt not in _NP_XTYPE or any(a.size != n for a in arrs):
        raise ValueError("host clients need equal-size float32 / float64 / int64 vectors of one type")
    _scratch(pinned, dev, *host_clients_scratch(nc, n, dt.itemsize))
    if any(len(st) != nc - 1 for st in streams):
        raise ValueError("every client needs n_clients - 1 streams")
    ptrs = (C.c_void_p * nc)(*[a.ctypes.data for a in arrs])
    ws = (C.c_double * nc)(*[float(w) for w in weights])
    sarr = make_streams([e for st in streams for e in st])
    out = np.empty(n, dtype=np.float64)
    digests = np.empty(nc, dtype=np.uint64)
    flags = C.c_uint32(0)
    ct = _NP_XTYPE[np.dtype(compute_dtype)]
    L.check(L.lib().sa_clients_host(ptrs, _NP_XTYPE[dt], ct, ws, nc, n, int(fxp_bits), sarr, float(divisor),
                                    _ptr(pinned), _ptr(dev), C.c_void_p(out.ctypes.data),
                                    C.c_void_p(digests.ctypes.data), C.byref(flags), C.c_void_p(_stream(dev))),
            "sa_clients_host")
    return out, digests, int(flags.value)


def mask_host_scratch(n: int, itemsize: int) -> tuple[int, int]:
    """(pinned bytes, device bytes) sa_mask_host needs."""
    n_pad, meta = _pad_meta(n, 2)  # the flag word + pad
    return n_pad * itemsize + (meta + n_pad) * 8, n_pad * itemsize + (meta + n_pad) * 8


def mask_host(x: np.ndarray, compute_dtype, streams: Sequence[tuple], pinned: torch.Tensor, dev: torch.Tensor, *,
              weight: float = 1.0, fxp_bits: int = 18):
    """One party's masked vector from a host array in ONE blocking call
    (sa_mask_host in include/sfl_sa.h) -> (uint64 host array, flag word)."""
    a = np.ascontiguousarray(x).reshape(-1)
    if a.dtype not in _NP_XTYPE:
        raise ValueError("mask_host takes float32 / float64 / int64 host arrays")
    n = int(a.size)
    _scratch(pinned, dev, *mask_host_scratch(n, a.dtype.itemsize))
    sarr = make_streams(streams)
    out = np.empty(n, dtype=np.uint64)
    flags = C.c_uint32(0)
    L.check(L.lib().sa_mask_host(C.c_void_p(a.ctypes.data), _NP_XTYPE[a.dtype], _NP_XTYPE[np.dtype(compute_dtype)],
                                 n, float(weight), int(fxp_bits), sarr, len(streams), _ptr(pinned), _ptr(dev),
                                 C.c_void_p(out.ctypes.data), C.byref(flags), C.c_void_p(_stream(dev))),
            "sa_mask_host")
    return out, int(flags.value)


def sum_decode_host_scratch(n_clients: int, n: int) -> tuple[int, int]:
    """(pinned bytes, device bytes) sa_sum_decode_host needs."""
    n_pad, meta = _pad_meta(n, n_clients)
    pin = (n_clients * n_pad + meta + n_pad) * 8
    return pin, pin + n_pad * 8


def sum_decode_host(masked: Sequence[np.ndarray], pinned: torch.Tensor, dev: torch.Tensor, *, fxp_bits: int = 18,
                    divisor: float = 1.0):
    """The server's step on host masked vectors in ONE blocking call
    (sa_sum_decode_host in include/sfl_sa.h) -> (decoded float64 host array,
    uint64 digests as received)."""
    arrs = [np.ascontiguousarray(m).view(np.uint64).reshape(-1) for m in masked]
    nc, n = len(arrs), int(arrs[0].size)
    if any(a.size != n for a in arrs):
        raise ValueError("masked vectors of different sizes")
    _scratch(pinned, dev, *sum_decode_host_scratch(nc, n))
    ptrs = (C.c_void_p * nc)(*[a.ctypes.data for a in arrs])
    out = np.empty(n, dtype=np.float64)
    digests = np.empty(nc, dtype=np.uint64)
    L.check(L.lib().sa_sum_decode_host(ptrs, nc, n, int(fxp_bits), float(divisor), _ptr(pinned), _ptr(dev),
                                       C.c_void_p(out.ctypes.data), C.c_void_p(digests.ctypes.data),
                                       C.c_void_p(_stream(dev))), "sa_sum_decode_host")
    return out, digests


def sum_f64(ins: Sequence[torch.Tensor], out: torch.Tensor) -> torch.Tensor:
    _require_gpu(out, *ins)
    ptrs = (C.c_void_p * len(ins))(*[t.data_ptr() for t in ins])
    L.check(L.lib().sa_sum_f64(ptrs, len(ins), out.numel(), _ptr(out), C.c_void_p(_stream(out))),
            "sa_sum_f64")
    return out


# ---------------------------------------------------------------------------
# GaussianModelDP pre-step (sa_sumsq_f32 / sa_dp_perturb_f32 / sa_mask_dp)
# ---------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def _fill_dp(d, sumsq, sumsq_layer, l2_norm_clip, noise_std, num_updates, counter0):
    """The fields sa_dp and sa_dp_secure share."""
    if counter0 % 4:
        raise ValueError("counter0 must be a multiple of 4")
    d.sumsq = sumsq.data_ptr()
    d.sumsq_layer = sumsq_layer.data_ptr() if sumsq_layer is not None else None
    d.l2_norm_clip = float(l2_norm_clip)
    d.noise_std = float(noise_std)
    d.num_updates = float(num_updates)
    d.counter0 = int(counter0)
    return d


def _dp_operands(who: str, x: torch.Tensor, out: torch.Tensor) -> None:
    _require_gpu(x, out)
    if x.dtype != torch.float32 or out.dtype != torch.float32 or out.numel() != x.numel():
        raise ValueError(f"{who}: float32 x and out of equal size")


def make_dp(sumsq: torch.Tensor, *, l2_norm_clip: float, noise_std: float, num_updates: float, key: int,
            counter0: int = 0, sumsq_layer: torch.Tensor | None = None) -> L.DP:
    d = _fill_dp(L.DP(), sumsq, sumsq_layer, l2_norm_clip, noise_std, num_updates, counter0)
    d.key = int(key) & _M64
    return d


def sumsq_f32(x: torch.Tensor, out: torch.Tensor, partials: torch.Tensor, *, accumulate: bool = False) -> torch.Tensor:
    """out[0] (+)= the layer's squared norm as the reference forms it (the
    float32 np.linalg.norm, squared in float64; sa_sumsq_f32)."""
    _require_gpu(x, out, partials)
    if x.dtype != torch.float32 or out.dtype != torch.float64 or partials.numel() < L.SA_DP_PARTIALS:
        raise ValueError("sumsq_f32: float32 x, float64 out, SA_DP_PARTIALS float64 partials")
    L.check(L.lib().sa_sumsq_f32(_ptr(x), x.numel(), _ptr(partials), _ptr(out), int(bool(accumulate)),
                                 C.c_void_p(_stream(out))), "sa_sumsq_f32")
    return out


def dp_perturb(x: torch.Tensor, out: torch.Tensor, dp: L.DP) -> torch.Tensor:
    _dp_operands("dp_perturb", x, out)
    L.check(L.lib().sa_dp_perturb_f32(_ptr(x), x.numel(), C.byref(dp), _ptr(out), C.c_void_p(_stream(out))),
            "sa_dp_perturb_f32")
    return out


def mask_dp(x: torch.Tensor, out: torch.Tensor, streams: Sequence[tuple], dp: L.DP, *, weight: float = 1.0,
            fxp_bits: int = 18, sum_accum: torch.Tensor | None = None, digest: torch.Tensor | None = None,
            flags: torch.Tensor | None = None) -> torch.Tensor:
    """sa_mask of the DP-perturbed float32 x, perturbation fused into the kernel."""
    _require_gpu(x, out, sum_accum, digest, flags)
    if x.dtype != torch.float32 or x.numel() != out.numel():
        raise ValueError("mask_dp: float32 x with out of equal size")
    sarr = make_streams(streams)
    L.check(L.lib().sa_mask_dp(_ptr(x), x.numel(), float(weight), int(fxp_bits), sarr, len(streams), C.byref(dp),
                               _ptr(out), _ptr(sum_accum), _ptr(digest), _ptr(flags), C.c_void_p(_stream(out))),
            "sa_mask_dp")
    return out


# ---------------------------------------------------------------------------
# FedSMP (sa_smp_*): the keyed mask, the masked scaled update d, its clipping
# norm, the fused upload and the unfused path's last step
# ---------------------------------------------------------------------------
def make_smp(key: int, counter0: int, threshold: int, divisor: float) -> L.SMP:
    if counter0 % 4:
        raise ValueError("counter0 must be a multiple of 4")
    return L.SMP(int(key) & _M64, int(counter0), int(threshold), float(divisor))


def _smp_operands(who: str, *ts: torch.Tensor) -> None:
    _require_gpu(*ts)
    if any(t.dtype != torch.float32 or t.numel() != ts[0].numel() for t in ts):
        raise ValueError(f"{who}: float32 tensors of equal size")


def smp_mask(smp: L.SMP, out: torch.Tensor) -> torch.Tensor:
    """out (uint8) = 1 where the element is kept (sa_smp_mask)."""
    _require_gpu(out)
    if out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("smp_mask: a contiguous uint8 out")
    L.check(L.lib().sa_smp_mask(C.byref(smp), out.numel(), _ptr(out), C.c_void_p(_stream(out))), "sa_smp_mask")
    return out


def smp_delta(w0: torch.Tensor, w1: torch.Tensor, smp: L.SMP, out: torch.Tensor) -> torch.Tensor:
    """out = kept ? (w1 - w0) / divisor : 0 (sa_smp_delta_f32)."""
    _smp_operands("smp_delta", w0, w1, out)
    L.check(L.lib().sa_smp_delta_f32(_ptr(w0), _ptr(w1), w0.numel(), C.byref(smp), _ptr(out),
                                     C.c_void_p(_stream(out))), "sa_smp_delta_f32")
    return out


def smp_sumsq(w0: torch.Tensor, w1: torch.Tensor, smp: L.SMP, out: torch.Tensor, partials: torch.Tensor, *,
              accumulate: bool = False) -> torch.Tensor:
    """out[0] (+)= sumsq_f32 of smp_delta's output, without storing it (sa_smp_sumsq_f32)."""
    _smp_operands("smp_sumsq", w0, w1)
    _require_gpu(out, partials)
    if out.dtype != torch.float64 or partials.dtype != torch.float64 or partials.numel() < L.SA_DP_PARTIALS:
        raise ValueError("smp_sumsq: float64 out, SA_DP_PARTIALS float64 partials")
    L.check(L.lib().sa_smp_sumsq_f32(_ptr(w0), _ptr(w1), w0.numel(), C.byref(smp), _ptr(partials), _ptr(out),
                                     int(bool(accumulate)), C.c_void_p(_stream(out))), "sa_smp_sumsq_f32")
    return out


def smp_perturb(w0: torch.Tensor, w1: torch.Tensor, smp: L.SMP, dp: L.DP | None, out: torch.Tensor) -> torch.Tensor:
    """out = kept ? w0 + (clip + noise of d) : w0 in one pass; ``dp`` None: no clip, no noise
    (sa_smp_perturb_f32).  out may be w1."""
    _smp_operands("smp_perturb", w0, w1, out)
    L.check(L.lib().sa_smp_perturb_f32(_ptr(w0), _ptr(w1), w0.numel(), C.byref(smp),
                                       None if dp is None else C.byref(dp), _ptr(out), C.c_void_p(_stream(out))),
            "sa_smp_perturb_f32")
    return out


def smp_finish(w0: torch.Tensor, t: torch.Tensor, smp: L.SMP, out: torch.Tensor) -> torch.Tensor:
    """out = kept ? w0 + t : w0 (sa_smp_finish_f32).  out may be t."""
    _smp_operands("smp_finish", w0, t, out)
    L.check(L.lib().sa_smp_finish_f32(_ptr(w0), _ptr(t), w0.numel(), C.byref(smp), _ptr(out),
                                      C.c_void_p(_stream(out))), "sa_smp_finish_f32")
    return out


# ---------------------------------------------------------------------------
# GaussianModelDP with ChaCha20 noise (sa_dp_perturb_secure_f32 and the two
# halves it is made of: sa_chacha20_keystream, sa_hb_normals_f64).  uint32
# words are carried as ``torch.int32`` tensors (same bits).
# ---------------------------------------------------------------------------
def make_dp_secure(sumsq: torch.Tensor, *, l2_norm_clip: float, noise_std: float, num_updates: float, key: bytes,
                   nonce: int, counter0: int = 0, sumsq_layer: torch.Tensor | None = None) -> L.DPSecure:
    d = _fill_dp(L.DPSecure(), sumsq, sumsq_layer, l2_norm_clip, noise_std, num_updates, counter0)
    d.key = L.chacha_key_words(key)
    d.nonce = int(nonce) & _M64
    return d


def dp_perturb_secure(x: torch.Tensor, out: torch.Tensor, dp: L.DPSecure) -> torch.Tensor:
    _dp_operands("dp_perturb_secure", x, out)
    L.check(L.lib().sa_dp_perturb_secure_f32(_ptr(x), x.numel(), C.byref(dp), _ptr(out), C.c_void_p(_stream(out))),
            "sa_dp_perturb_secure_f32")
    return out


def chacha20_keystream(key: bytes, nonce: int, block0: int, out: torch.Tensor) -> torch.Tensor:
    """out (int32, 16 words per block) = the ChaCha20 blocks block0 .. of (key, nonce)."""
    _require_gpu(out)
    if out.dtype != torch.int32 or out.numel() % 16:
        raise ValueError("chacha20_keystream: an int32 out of 16 words per block")
    L.check(L.lib().sa_chacha20_keystream(L.chacha_key_words(key), int(nonce) & _M64, int(block0) & _M64,
                                          out.numel() // 16, _ptr(out), C.c_void_p(_stream(out))),
            "sa_chacha20_keystream")
    return out


def hb_normals(words: torch.Tensor, sigma: float, out: torch.Tensor) -> torch.Tensor:
    """out[i] (float64) = the normal of standard deviation sigma that the four
    words words[4 i .. 4 i + 3] (int32) make (sa_hb_normals_f64)."""
    _require_gpu(words, out)
    if words.dtype != torch.int32 or out.dtype != torch.float64 or words.numel() != 4 * out.numel():
        raise ValueError("hb_normals: int32 words, four per float64 element of out")
    L.check(L.lib().sa_hb_normals_f64(_ptr(words), out.numel(), float(sigma), _ptr(out), C.c_void_p(_stream(out))),
            "sa_hb_normals_f64")
    return out


# ---------------------------------------------------------------------------
# the compression kernels (sa_stc, sa_scr, sa_coo_*, sa_quant_*): what their
# wrappers share
# ---------------------------------------------------------------------------
def _float_xtype(what: str, dtype) -> int:
    if dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{what}: float32 or float64, not {dtype}")
    return xtype_of(dtype)


def _scratch_bytes(what: str, entry: str, dims: Sequence[int], dtype) -> int:
    """The library's ``entry(*dims, x_type)``: bytes of device scratch."""
    xt = _float_xtype(what, dtype)
    rc = getattr(L.lib(), entry)(*(int(d) for d in dims), xt)
    if rc < 0:
        L.check(rc, entry)
    return rc


def _require_scratch(what: str, scratch: torch.Tensor, need: int, sized_by: str) -> None:
    if scratch.numel() * scratch.element_size() < need:
        raise ValueError(f"{what}: scratch smaller than {sized_by}")


# ---------------------------------------------------------------------------
# sparse ternary compression (sa_stc; fed_stc's worker and server halves)
# ---------------------------------------------------------------------------
def stc_scratch_bytes(n: int, dtype: torch.dtype) -> int:
    """Bytes of device scratch ``stc`` needs for ``n`` elements of ``dtype``."""
    return _scratch_bytes("stc", "sa_stc_scratch_bytes", (n,), dtype)


def stc(a: torch.Tensor, b: torch.Tensor | None, r: torch.Tensor | None, mask_num: int, sparse_out: torch.Tensor,
        res_out: torch.Tensor, *, acc: torch.Tensor | None = None, mu_out: torch.Tensor | None = None,
        scratch: torch.Tensor) -> torch.Tensor:
    """u = (a - b) + r; mask the ``mask_num`` elements of smallest |u| (ties:
    lower index first); sparse_out = mu * sign(u_masked) with mu the mean of
    the survivors' |u|; res_out = u - sparse_out (may be ``r`` itself);
    acc += sparse_out.  ``b``, ``r``, ``acc``, ``mu_out`` (one element) are
    optional.  See sa_stc in include/sfl_sa.h."""
    _require_gpu(a, b, r, sparse_out, res_out, acc, mu_out, scratch)
    n = a.numel()
    for t in (a, b, r, sparse_out, res_out, acc):
        if t is not None and (t.dtype != a.dtype or t.numel() != n or not t.is_contiguous()):
            raise ValueError("stc: contiguous tensors of one dtype and size")
    if mu_out is not None and (mu_out.dtype != a.dtype or mu_out.numel() < 1):
        raise ValueError("stc: mu_out is one element of the data's dtype")
    _require_scratch("stc", scratch, stc_scratch_bytes(n, a.dtype), "stc_scratch_bytes(n, dtype)")
    if not 0 <= int(mask_num) <= n:
        raise ValueError("stc: mask_num outside [0, n]")
    L.check(L.lib().sa_stc(_ptr(a), _ptr(b), _ptr(r), xtype_of(a.dtype), n, int(mask_num), _ptr(sparse_out),
                           _ptr(res_out), _ptr(acc), _ptr(mu_out), _ptr(scratch), C.c_void_p(_stream(a))),
            "sa_stc")
    return sparse_out


# ---------------------------------------------------------------------------
# structure-wise update pruning (sa_scr; fed_scr's worker)
# ---------------------------------------------------------------------------
def scr_scratch_bytes(shape3: Sequence[int], dtype: torch.dtype) -> int:
    """Bytes of device scratch ``scr`` needs for a ``[rows, cols, inner]`` tensor of ``dtype``."""
    rows, cols, inner = shape3
    return _scratch_bytes("scr", "sa_scr_scratch_bytes", (rows, cols, inner), dtype)


def scr(a: torch.Tensor, b: torch.Tensor | None, r: torch.Tensor | None, shape3: Sequence[int], threshold: float,
        sparse_out: torch.Tensor, res_out: torch.Tensor | None = None, *, stats_out: torch.Tensor | None = None,
        scratch: torch.Tensor) -> torch.Tensor:
    """u = (a - b) + r seen as ``shape3 = [rows, cols, inner]``; rows, then
    columns over the kept rows, whose float64 sum of |u| relative to the
    largest such sum is <= ``threshold`` are set to +0 in sparse_out;
    res_out = u - sparse_out (may be ``r`` itself).  ``b``, ``r``,
    ``res_out`` and ``stats_out`` (two uint32 / int32: dropped rows, dropped
    columns) are optional.  See sa_scr in include/sfl_sa.h."""
    _require_gpu(a, b, r, sparse_out, res_out, stats_out, scratch)
    rows, cols, inner = (int(d) for d in shape3)
    n = a.numel()
    if min(rows, cols, inner) < 1 or rows * cols * inner != n:
        raise ValueError("scr: shape3 is [rows, cols, inner] with rows * cols * inner == a.numel() > 0")
    for t in (a, b, r, sparse_out, res_out):
        if t is not None and (t.dtype != a.dtype or t.numel() != n or not t.is_contiguous()):
            raise ValueError("scr: contiguous tensors of one dtype and size")
    if stats_out is not None and (stats_out.element_size() != 4 or stats_out.numel() < 2
                                  or not stats_out.is_contiguous()):
        raise ValueError("scr: stats_out is two 32-bit integers")
    _require_scratch("scr", scratch, scr_scratch_bytes((rows, cols, inner), a.dtype),
                     "scr_scratch_bytes(shape3, dtype)")
    L.check(L.lib().sa_scr(_ptr(a), _ptr(b), _ptr(r), xtype_of(a.dtype), rows, cols, inner, float(threshold),
                           _ptr(sparse_out), _ptr(res_out), _ptr(stats_out), _ptr(scratch),
                           C.c_void_p(_stream(a))),
            "sa_scr")
    return sparse_out


# ---------------------------------------------------------------------------
# COO transport and the sparse server sum (sa_coo_*; utils/sparse.py and
# SparsePlainAggregator on top)
# ---------------------------------------------------------------------------
def _coo_words(what: str, name: str, t: torch.Tensor, words: int) -> None:
    if t.dtype != torch.int32 or t.numel() < words or not t.is_contiguous():
        raise ValueError(f"{what}: {name} is {words} contiguous int32 word{'s' if words > 1 else ''}")


def _coo_payload(what: str, index: torch.Tensor, data: torch.Tensor) -> int:
    xt = _float_xtype(what, data.dtype)
    if index.dtype != torch.int32 or index.dim() != 1 or data.dim() != 1 or index.numel() != data.numel() \
            or not index.is_contiguous() or not data.is_contiguous():
        raise ValueError(f"{what}: index (int32) and data are flat contiguous tensors of one length")
    return xt


def coo_scratch_bytes(n: int, dtype: torch.dtype) -> int:
    """Bytes of device scratch ``coo_count`` / ``coo_fill`` need for ``n`` elements of ``dtype``."""
    return _scratch_bytes("coo_scratch_bytes", "sa_coo_scratch_bytes", (n,), dtype)


def coo_flag(device) -> torch.Tensor:
    """A fresh flag record for ``coo_fill`` / ``coo_decode`` / ``coo_axpy``:
    no bit set, no offending position (``[0, -1]`` as int32)."""
    flag = torch.zeros(2, dtype=torch.int32, device=device)
    flag[1:].fill_(-1)  # a fill kernel: indexed assignment of a Python scalar copies it from the host
    return flag


def coo_count(x: torch.Tensor, scratch: torch.Tensor, nnz_out: torch.Tensor) -> torch.Tensor:
    """The encode's first pass: the number of non-zeros of ``x`` (by the bit
    rule) into the device word ``nnz_out`` (one int32), and every wave's
    first rank into ``scratch`` for ``coo_fill``.  See sa_coo_count in
    include/sfl_sa.h."""
    _require_gpu(x, scratch, nnz_out)
    xt = _float_xtype("coo_count", x.dtype)
    if not x.is_contiguous():
        raise ValueError("coo_count: a contiguous tensor")
    _coo_words("coo_count", "nnz_out", nnz_out, 1)
    _require_scratch("coo_count", scratch, coo_scratch_bytes(x.numel(), x.dtype), "coo_scratch_bytes(n, dtype)")
    L.check(L.lib().sa_coo_count(_ptr(x), xt, x.numel(), _ptr(scratch), _ptr(nnz_out), C.c_void_p(_stream(x))),
            "sa_coo_count")
    return nnz_out


def coo_fill(x: torch.Tensor, scratch: torch.Tensor, index_out: torch.Tensor, data_out: torch.Tensor,
             flag: torch.Tensor, *, cap: int | None = None) -> None:
    """The encode's second pass, after ``coo_count`` of the same ``x`` into
    the same ``scratch``: the flat indices (int32, ascending) and the values
    of the non-zeros.  At most ``cap`` entries (default: the outputs' length)
    are stored; a count other than ``cap`` sets ``SA_COO_BAD_COUNT`` in
    ``flag``."""
    _require_gpu(x, scratch, index_out, data_out, flag)
    xt = _float_xtype("coo_fill", x.dtype)
    if not x.is_contiguous():
        raise ValueError("coo_fill: a contiguous tensor")
    if data_out.dtype != x.dtype:
        raise ValueError("coo_fill: data_out has the tensor's dtype")
    _coo_payload("coo_fill", index_out, data_out)
    _coo_words("coo_fill", "flag", flag, 2)
    cap = index_out.numel() if cap is None else int(cap)
    if not 0 <= cap <= min(index_out.numel(), x.numel()):
        raise ValueError("coo_fill: cap outside [0, min(len(index_out), n)]")
    _require_scratch("coo_fill", scratch, coo_scratch_bytes(x.numel(), x.dtype), "coo_scratch_bytes(n, dtype)")
    L.check(L.lib().sa_coo_fill(_ptr(x), xt, x.numel(), _ptr(scratch), _ptr(index_out), _ptr(data_out), cap,
                                _ptr(flag), C.c_void_p(_stream(x))), "sa_coo_fill")


def coo_decode(index: torch.Tensor, data: torch.Tensor, dense_out: torch.Tensor, flag: torch.Tensor) -> torch.Tensor:
    """dense_out = 0, then dense_out[index[i]] = data[i] for every entry
    inside the tensor; what was wrong with the payload goes into ``flag``."""
    _require_gpu(index, data, dense_out, flag)
    xt = _coo_payload("coo_decode", index, data)
    if dense_out.dtype != data.dtype or not dense_out.is_contiguous():
        raise ValueError("coo_decode: dense_out is contiguous and has the data's dtype")
    if index.numel() > dense_out.numel():
        raise ValueError("coo_decode: more entries than the tensor has elements")
    _coo_words("coo_decode", "flag", flag, 2)
    L.check(L.lib().sa_coo_decode(_ptr(index), _ptr(data), xt, index.numel(), dense_out.numel(), _ptr(dense_out),
                                  _ptr(flag), C.c_void_p(_stream(dense_out))), "sa_coo_decode")
    return dense_out


def coo_axpy(index: torch.Tensor, data: torch.Tensor, w: float, acc: torch.Tensor, flag: torch.Tensor) -> torch.Tensor:
    """acc[index[i]] = acc[index[i]] + A(data[i]) * A(w), multiply and add
    rounded separately, ``A`` the accumulator's type (float32 data: float32 or
    float64; float64 data: float64).  Validates like ``coo_decode``."""
    _require_gpu(index, data, acc, flag)
    xt = _coo_payload("coo_axpy", index, data)
    at = _float_xtype("coo_axpy", acc.dtype)
    if data.dtype == torch.float64 and acc.dtype == torch.float32:
        raise TypeError("coo_axpy: float64 data needs a float64 accumulator")
    if not acc.is_contiguous():
        raise ValueError("coo_axpy: a contiguous accumulator")
    if index.numel() > acc.numel():
        raise ValueError("coo_axpy: more entries than the tensor has elements")
    _coo_words("coo_axpy", "flag", flag, 2)
    L.check(L.lib().sa_coo_axpy(_ptr(index), _ptr(data), xt, index.numel(), float(w), _ptr(acc), at, acc.numel(),
                                _ptr(flag), C.c_void_p(_stream(acc))), "sa_coo_axpy")
    return acc


def coo_finish(acc: torch.Tensor, divisor: float) -> torch.Tensor:
    """acc[i] = acc[i] / A(divisor) in place."""
    _require_gpu(acc)
    at = _float_xtype("coo_finish", acc.dtype)
    if not acc.is_contiguous():
        raise ValueError("coo_finish: a contiguous accumulator")
    L.check(L.lib().sa_coo_finish(_ptr(acc), at, acc.numel(), float(divisor), C.c_void_p(_stream(acc))),
            "sa_coo_finish")
    return acc


def coo_gather(index: torch.Tensor, x: torch.Tensor, data_out: torch.Tensor, flag: torch.Tensor) -> torch.Tensor:
    """data_out[i] = x[index[i]]: a tensor's values at a mask's positions.  An
    index outside the tensor is not used and goes into ``flag`` like a
    payload's.  See sa_coo_gather in include/sfl_sa.h."""
    _require_gpu(index, x, data_out, flag)
    xt = _coo_payload("coo_gather", index, data_out)
    if x.dtype != data_out.dtype or not x.is_contiguous():
        raise ValueError("coo_gather: x is contiguous and has data_out's dtype")
    if index.numel() > x.numel():
        raise ValueError("coo_gather: more entries than the tensor has elements")
    _coo_words("coo_gather", "flag", flag, 2)
    L.check(L.lib().sa_coo_gather(_ptr(index), index.numel(), _ptr(x), xt, x.numel(), _ptr(data_out), _ptr(flag),
                                  C.c_void_p(_stream(x))), "sa_coo_gather")
    return data_out


# ---------------------------------------------------------------------------
# top-k sparsification (sa_topk_*; utils/sparse_compressor.py on top)
# ---------------------------------------------------------------------------
def topk_scratch_bytes(n: int, dtype: torch.dtype) -> int:
    """Bytes of device scratch ``topk_select`` / ``topk_fill`` share for ``n`` keys of ``dtype``."""
    return _scratch_bytes("topk_scratch_bytes", "sa_topk_scratch_bytes", (n,), dtype)


def _topk_keys(what: str, keys: torch.Tensor, k: int, scratch: torch.Tensor) -> int:
    kt = _float_xtype(what, keys.dtype)
    if keys.dim() != 1 or not keys.is_contiguous():
        raise ValueError(f"{what}: keys is a flat contiguous tensor")
    if not 0 <= int(k) <= keys.numel():
        raise ValueError(f"{what}: k outside [0, n]")
    _require_scratch(what, scratch, topk_scratch_bytes(keys.numel(), keys.dtype), "topk_scratch_bytes(n, dtype)")
    return kt


def topk_select(keys: torch.Tensor, k: int, scratch: torch.Tensor) -> None:
    """The threshold of the ``k`` largest magnitudes of ``keys`` (ties: the
    higher indices are kept) and every wave's tie and output ranks into
    ``scratch``, for ``topk_fill``.  See sa_topk_select in include/sfl_sa.h."""
    _require_gpu(keys, scratch)
    kt = _topk_keys("topk_select", keys, k, scratch)
    L.check(L.lib().sa_topk_select(_ptr(keys), kt, keys.numel(), int(k), _ptr(scratch), C.c_void_p(_stream(keys))),
            "sa_topk_select")


def topk_fill(keys: torch.Tensor, x: torch.Tensor, k: int, scratch: torch.Tensor, index_out: torch.Tensor,
              data_out: torch.Tensor, flag: torch.Tensor) -> None:
    """After ``topk_select`` of the same ``keys`` and ``k`` into the same
    ``scratch``: the kept flat indices (int32, ascending) and ``x`` at them.
    ``x`` is ``keys`` itself or another flat tensor of its length; a total
    other than ``k`` sets ``SA_COO_BAD_COUNT`` in ``flag``."""
    _require_gpu(keys, x, scratch, index_out, data_out, flag)
    kt = _topk_keys("topk_fill", keys, k, scratch)
    if x.dim() != 1 or x.numel() != keys.numel() or not x.is_contiguous():
        raise ValueError("topk_fill: x is a flat contiguous tensor of keys' length")
    if data_out.dtype != x.dtype:
        raise ValueError("topk_fill: data_out has x's dtype")
    xt = _coo_payload("topk_fill", index_out, data_out)
    if index_out.numel() < int(k):
        raise ValueError("topk_fill: index_out and data_out hold k entries")
    _coo_words("topk_fill", "flag", flag, 2)
    L.check(L.lib().sa_topk_fill(_ptr(keys), kt, _ptr(x), xt, keys.numel(), int(k), _ptr(scratch), _ptr(index_out),
                                 _ptr(data_out), _ptr(flag), C.c_void_p(_stream(keys))), "sa_topk_fill")


def topk_random_keys(seed: int, keys_out: torch.Tensor) -> torch.Tensor:
    """RandomSparse's 63-bit keys under ``seed`` into ``keys_out`` (float64
    or int64: 8-byte words), element ``e`` from the Philox words ``2e`` and
    ``2e + 1``.  See sa_topk_random_keys in include/sfl_sa.h."""
    _require_gpu(keys_out)
    if keys_out.element_size() != 8 or keys_out.dim() != 1 or not keys_out.is_contiguous():
        raise ValueError("topk_random_keys: keys_out is a flat contiguous tensor of 8-byte words")
    L.check(L.lib().sa_topk_random_keys(int(seed) & 0xFFFFFFFFFFFFFFFF, keys_out.numel(), _ptr(keys_out),
                                        C.c_void_p(_stream(keys_out))), "sa_topk_random_keys")
    return keys_out


# ---------------------------------------------------------------------------
# quantized compressors (sa_quant_*; utils/quantized.py on top)
# ---------------------------------------------------------------------------
_QUANT_CODES = {torch.int8: 1, torch.int16: 2}


def _quant_pair(what: str, x: torch.Tensor, q: torch.Tensor, codes=_QUANT_CODES) -> tuple[int, int]:
    """(x_type, q_bytes) of a float tensor and its codes: contiguous, one length, one device."""
    _require_gpu(x, q)
    xt = _float_xtype(what, x.dtype)
    if q.dtype not in codes:
        raise TypeError(f"{what}: the codes are {' or '.join(str(d) for d in codes)}, not {q.dtype}")
    if not x.is_contiguous() or not q.is_contiguous() or x.numel() != q.numel() or x.device != q.device:
        raise ValueError(f"{what}: the data and the codes are contiguous tensors of one length on one device")
    return xt, codes[q.dtype]


def quant_scratch_bytes(n: int, dtype: torch.dtype) -> int:
    """Bytes of device scratch ``quant_range`` needs for ``n`` elements of ``dtype``."""
    return _scratch_bytes("quant_scratch_bytes", "sa_quant_scratch_bytes", (n,), dtype)


def quant_range(x: torch.Tensor, scratch: torch.Tensor, out3: torch.Tensor) -> torch.Tensor:
    """``out3 = (min, max, max|x|)`` of ``x``, three elements of its dtype on
    the device, NaN-propagating.  See sa_quant_range in include/sfl_sa.h."""
    _require_gpu(x, scratch, out3)
    xt = _float_xtype("quant_range", x.dtype)
    if not x.is_contiguous():
        raise ValueError("quant_range: a contiguous tensor")
    if out3.dtype != x.dtype or out3.numel() < 3 or not out3.is_contiguous():
        raise ValueError("quant_range: out3 is three contiguous elements of the data's dtype")
    _require_scratch("quant_range", scratch, quant_scratch_bytes(x.numel(), x.dtype),
                     "quant_scratch_bytes(n, dtype)")
    L.check(L.lib().sa_quant_range(_ptr(x), xt, x.numel(), _ptr(scratch), _ptr(out3), C.c_void_p(_stream(x))),
            "sa_quant_range")
    return out3


def quant_affine(x: torch.Tensor, mode: int, p0: float, p1: float, qmin: int, qmax: int,
                 q_out: torch.Tensor) -> torch.Tensor:
    """The codes of ``x`` into ``q_out`` (int8 or int16).  ``mode``
    ``L.SA_QUANT_ZERO_POINT``: ``p0 = scale``, ``p1 = z``; ``L.SA_QUANT_LSTM``:
    ``p0 = q``, ``p1 = rqm`` rounded to the data's type.  See sa_quant_affine."""
    xt, qb = _quant_pair("quant_affine", x, q_out)
    L.check(L.lib().sa_quant_affine(_ptr(x), xt, x.numel(), int(mode), float(p0), float(p1), int(qmin), int(qmax),
                                    _ptr(q_out), qb, C.c_void_p(_stream(x))), "sa_quant_affine")
    return q_out


def dequant_affine(q: torch.Tensor, mode: int, p0: float, p1: float, out: torch.Tensor) -> torch.Tensor:
    """``out`` (float32 / float64) from the codes ``q``; the parameters as in ``quant_affine``."""
    xt, qb = _quant_pair("dequant_affine", out, q)
    L.check(L.lib().sa_dequant_affine(_ptr(q), qb, q.numel(), int(mode), float(p0), float(p1), xt, _ptr(out),
                                      C.c_void_p(_stream(out))), "sa_dequant_affine")
    return out


_FP8_CODES = {torch.int8: 1}


def quant_fp8(x: torch.Tensor, scale: float, mant_len: int, exp_offset: int, q_out: torch.Tensor) -> torch.Tensor:
    """The fp8 codes of ``x`` into ``q_out`` (int8).  See sa_quant_fp8."""
    xt, _ = _quant_pair("quant_fp8", x, q_out, _FP8_CODES)
    L.check(L.lib().sa_quant_fp8(_ptr(x), xt, x.numel(), float(scale), int(mant_len), int(exp_offset), _ptr(q_out),
                                 C.c_void_p(_stream(x))), "sa_quant_fp8")
    return q_out


def dequant_fp8(q: torch.Tensor, scale: float, mant_len: int, exp_offset: int, out: torch.Tensor) -> torch.Tensor:
    """``out`` (float32 / float64) from the fp8 codes ``q`` (int8)."""
    xt, _ = _quant_pair("dequant_fp8", out, q, _FP8_CODES)
    L.check(L.lib().sa_dequant_fp8(_ptr(q), q.numel(), float(scale), int(mant_len), int(exp_offset), xt, _ptr(out),
                                   C.c_void_p(_stream(out))), "sa_dequant_fp8")
    return out


# ---------------------------------------------------------------------------
# numpy's rejection re-draw (after SA_FLAG_PRG_REJECT; never on the hot path)
# ---------------------------------------------------------------------------
U64_MAX = (1 << 64) - 1


def find_zero_draws(gens: Sequence, n: int, device) -> list:
    """For each generator, the first raw draw index in [0, n) whose PCG64
    output is 0 (numpy's Generator.integers rejects it), or None."""
    if not gens:
        return []
    first = torch.full((len(gens),), -1, dtype=torch.int64, device=device)  # all ones = UINT64_MAX
    arr = (L.PCG64 * len(gens))(*gens)
    L.check(L.lib().sa_pcg64_find_zero(arr, len(gens), int(n), _ptr(first), C.c_void_p(_stream(first))),
            "sa_pcg64_find_zero")
    return [None if v == U64_MAX else int(v) for v in as_u64(first).tolist()]


def stream_shift(out: torch.Tensor, gen, sign: int, k: int, shift: int) -> torch.Tensor:
    """out[e] += sign * (raw[e+shift] - raw[e+shift-1]) for e >= k (in place)."""
    _require_gpu(out)
    g = L.PCG64(gen.state, gen.inc)
    L.check(L.lib().sa_stream_shift(_ptr(out), out.numel(), C.byref(g), int(sign), int(k), int(shift),
                                    C.c_void_p(_stream(out))), "sa_stream_shift")
    return out


def xor_digest(v: torch.Tensor, digest: torch.Tensor) -> torch.Tensor:
    """digest[0] ^= XOR of every uint64 element of v."""
    _require_gpu(v, digest)
    L.check(L.lib().sa_xor_u64(_ptr(v), v.numel(), _ptr(digest), C.c_void_p(_stream(v))), "sa_xor_u64")
    return digest


def rejected_draws(gen, n: int, device, first: int | None = -1) -> tuple[list, int]:
    """numpy's Generator.integers over n elements from ``gen``: the
    (element, shift) points where a rejected raw 0 moves the stream one raw
    draw further (element e >= k uses raw[e + shift]), and the total number
    of raw draws consumed (n + rejections).  ``first``: the stream's first
    zero in [0, n) when already searched (None: there is none)."""
    if first is None:
        return [], n
    pts, e0, s = [], 0, 0
    if first != -1:
        e0, s = first, 1
        pts.append((e0, s))
    while e0 < n:
        # elements >= e0 use raw[e + s]: search raw[e0 + s, n + s)
        z = find_zero_draws([L.pcg64_advance(gen, e0 + s)], n - e0, device)[0]
        if z is None:
            break
        e0, s = e0 + z, s + 1
        pts.append((e0, s))
    return pts, n + s


def rejected_draws_many(gens: Sequence, n: int, device) -> list:
    """``rejected_draws`` for many streams: the first zero of every stream is
    searched by ONE sa_pcg64_find_zero call (up to 64 generators per launch
    inside it) and one host sync; only the streams with a hit are followed
    further."""
    first = find_zero_draws(list(gens), n, device)
    return [rejected_draws(g, n, device, first=f) for g, f in zip(gens, first)]


def stream_shifts(out: torch.Tensor, gen, sign: int, pts: Sequence[tuple]) -> torch.Tensor:
    """``stream_shift`` at every (element, shift) point ``rejected_draws`` found on one stream."""
    for k, shift in pts:
        stream_shift(out, gen, sign, k, shift)
    return out


# ---------------------------------------------------------------------------
# QuantizedKmeans (sa_kmeans_*, sa_dequant_lut; utils/quantized.py on top)
# ---------------------------------------------------------------------------
def kmeans_scratch_bytes(n: int, dtype: torch.dtype) -> int:
    """Bytes of device scratch a fit of ``n`` elements of ``dtype`` needs: the
    histogram (``SA_KMEANS_BINS`` words), then the state block."""
    return _scratch_bytes("kmeans_scratch_bytes", "sa_kmeans_scratch_bytes", (n,), dtype)


def _kmeans_x(what: str, x: torch.Tensor, k: int | None = None) -> int:
    _require_gpu(x)
    xt = _float_xtype(what, x.dtype)
    if not x.is_contiguous():
        raise ValueError(f"{what}: a contiguous tensor")
    if k is not None and not 2 <= int(k) <= L.SA_KMEANS_MAX_K:
        raise ValueError(f"{what}: k must be in 2..{L.SA_KMEANS_MAX_K}, got {k}")
    return xt


def _kmeans_state(what: str, state: torch.Tensor) -> None:
    _require_gpu(state)
    if state.numel() * state.element_size() < L.SA_KMEANS_STATE_BYTES or not state.is_contiguous() \
            or state.data_ptr() % 8:
        raise ValueError(f"{what}: the state is {L.SA_KMEANS_STATE_BYTES} contiguous, 8-byte aligned bytes")


def kmeans_hist(x: torch.Tensor, mn: float, s: float, hist: torch.Tensor) -> torch.Tensor:
    """The 4096-bin histogram of the image of ``x`` into ``hist`` (int32 words
    that carry uint32 counts).  See sa_kmeans_hist in include/sfl_sa.h."""
    xt = _kmeans_x("kmeans_hist", x)
    _require_gpu(hist)
    _coo_words("kmeans_hist", "hist", hist, L.SA_KMEANS_BINS)
    L.check(L.lib().sa_kmeans_hist(_ptr(x), xt, x.numel(), float(mn), float(s), _ptr(hist), C.c_void_p(_stream(x))),
            "sa_kmeans_hist")
    return hist


def kmeans_step(x: torch.Tensor, mn: float, s: float, k: int, steps: int, state: torch.Tensor) -> torch.Tensor:
    """``steps`` Lloyd steps on ``state``, enqueued back to back; a step after
    the one that moved no centre does nothing.  See sa_kmeans_step."""
    xt = _kmeans_x("kmeans_step", x, k)
    _kmeans_state("kmeans_step", state)
    L.check(L.lib().sa_kmeans_step(_ptr(x), xt, x.numel(), float(mn), float(s), int(k), int(steps), _ptr(state),
                                   C.c_void_p(_stream(x))), "sa_kmeans_step")
    return state


def kmeans_labels(x: torch.Tensor, mn: float, s: float, k: int, state: torch.Tensor, offset: int,
                  q_out: torch.Tensor) -> torch.Tensor:
    """``q_out`` (int8 / int16) = the label of every element under the state's
    centres, minus ``offset``.  See sa_kmeans_labels."""
    xt, qb = _quant_pair("kmeans_labels", x, q_out)
    _kmeans_x("kmeans_labels", x, k)
    _kmeans_state("kmeans_labels", state)
    L.check(L.lib().sa_kmeans_labels(_ptr(x), xt, x.numel(), float(mn), float(s), int(k), _ptr(state), int(offset),
                                     _ptr(q_out), qb, C.c_void_p(_stream(x))), "sa_kmeans_labels")
    return q_out


def dequant_lut(q: torch.Tensor, lut: torch.Tensor, offset: int, out: torch.Tensor, flag: torch.Tensor) -> torch.Tensor:
    """``out[i] = lut[q[i] + offset]``; a label outside ``[0, len(lut))`` gives
    0 and goes into ``flag`` (a ``coo_flag`` record).  See sa_dequant_lut."""
    xt, qb = _quant_pair("dequant_lut", out, q)
    _require_gpu(lut, flag)
    k = lut.numel()
    if lut.dtype != out.dtype or not lut.is_contiguous() or not 2 <= k <= L.SA_KMEANS_MAX_K:
        raise ValueError(f"dequant_lut: lut is 2..{L.SA_KMEANS_MAX_K} contiguous values of the output's dtype")
    _coo_words("dequant_lut", "flag", flag, 2)
    L.check(L.lib().sa_dequant_lut(_ptr(q), qb, q.numel(), _ptr(lut), k, int(offset), xt, _ptr(out), _ptr(flag),
                                   C.c_void_p(_stream(out))), "sa_dequant_lut")
    return out


# ---------------------------------------------------------------------------
# FlameAggregator (sa_flame_*; security/aggregation/flame_aggregator.py on top)
# ---------------------------------------------------------------------------
def flame_stat_count(n_clients: int) -> int:
    """The statistics of ``n_clients`` clients: the Gram matrix's packed upper
    triangle, then the squared update norms."""
    return n_clients * (n_clients + 1) // 2 + n_clients


def flame_scratch_bytes(n: int, n_clients: int, dtype: torch.dtype) -> int:
    """Bytes of device scratch ``flame_stats`` needs for ``n`` elements of ``n_clients`` clients."""
    return _scratch_bytes("flame_scratch_bytes", "sa_flame_scratch_bytes", (n, n_clients), dtype)


def _flame_table(what: str, xs: Sequence, like: torch.Tensor) -> C.Array:
    """The host table of the clients' device pointers.  An entry is a tensor
    of ``like``'s size and dtype, or -- handed to the library as it is, which
    refuses what it cannot take -- ``None`` or an address."""
    table = (C.c_void_p * max(1, len(xs)))()
    for i, x in enumerate(xs):
        if isinstance(x, torch.Tensor):
            _require_gpu(x)
            if x.dtype != like.dtype or x.numel() != like.numel() or not x.is_contiguous() or x.device != like.device:
                raise ValueError(f"{what}: client {i}'s tensor is contiguous, of the median's size, dtype and device")
            table[i] = x.data_ptr()
        else:
            table[i] = x
    return table


def flame_stats(xs: Sequence, median_out: torch.Tensor, scratch: torch.Tensor, stats: torch.Tensor, *,
                accumulate: bool = False) -> torch.Tensor:
    """The element-wise median of the clients' tensors ``xs`` into
    ``median_out``; their Gram matrix and squared update norms into ``stats``
    (float64, ``flame_stat_count(len(xs))`` values), added to what is there
    with ``accumulate``.  The client count, the element type and the pointers
    are judged by the library.  See sa_flame_stats in include/sfl_sa.h."""
    _require_gpu(median_out, scratch, stats)
    c, n = len(xs), median_out.numel()
    if not median_out.is_contiguous() or not stats.is_contiguous() or stats.dtype != torch.float64:
        raise ValueError("flame_stats: contiguous tensors; stats is float64")
    xt = _XTYPE.get(median_out.dtype, -1)
    if 1 <= c <= L.SA_FLAME_MAX_CLIENTS and xt in (L.SA_F32, L.SA_F64):
        if stats.numel() < flame_stat_count(c):
            raise ValueError("flame_stats: stats smaller than flame_stat_count(len(xs))")
        _require_scratch("flame_stats", scratch, flame_scratch_bytes(n, c, median_out.dtype),
                         "flame_scratch_bytes(n, n_clients, dtype)")
    table = _flame_table("flame_stats", xs, median_out)
    L.check(L.lib().sa_flame_stats(table, c, xt, n, _ptr(median_out), _ptr(scratch), _ptr(stats), int(bool(accumulate)),
                                   C.c_void_p(_stream(median_out))), "sa_flame_stats")
    return stats


def flame_combine(xs: Sequence, scales: Sequence[float], weights: Sequence[float], keep: Sequence[bool],
                  median: torch.Tensor, divisor: float, out: torch.Tensor) -> torch.Tensor:
    """``out`` (float64) = the weighted average of the kept clients' clipped
    models ``median + (x - median) * scale``, divided by ``divisor``.  A
    client with ``keep[i]`` false crosses the C-ABI with a NaN weight, the
    entry's mark of a dropped client: its tensor is never read.  See
    sa_flame_combine in include/sfl_sa.h."""
    _require_gpu(median, out)
    c, n = len(xs), median.numel()
    if not (len(scales) == len(weights) == len(keep) == c):
        raise ValueError("flame_combine: one scale, weight and keep flag per client")
    if not median.is_contiguous() or not out.is_contiguous() or out.dtype != torch.float64 or out.numel() != n \
            or out.device != median.device:
        raise ValueError("flame_combine: out is contiguous float64 of the median's size, on its device")
    table = _flame_table("flame_combine", xs, median)
    s = (C.c_double * max(1, c))(*[float(v) for v in scales])
    w = (C.c_double * max(1, c))(*[float(v) if k else float("nan") for v, k in zip(weights, keep)])
    L.check(L.lib().sa_flame_combine(table, s, w, c, _XTYPE.get(median.dtype, -1), n, _ptr(median), float(divisor),
                                     _ptr(out), C.c_void_p(_stream(median))), "sa_flame_combine")
    return out
