"""Update compression.  Sparse ternary compression (STC), the counterpart of the reference's
``sfl/utils/compressor``: ``STCSparse`` (``sparse_compressor.py:142-179``)
and the fused step the ``fed_stc`` worker and server run around it
(``fed_stc.py:97-125``, ``compress.py:28-42``).

The definition, for one tensor flattened to ``n`` elements of type T and
``mask_num = round(sparse_rate * n)`` (Python's ``round``):

1. ``u = (a - b) + r``, every operation rounded in T; an absent ``b`` or ``r``
   means the operation is not performed.
2. The ``mask_num`` elements of smallest ``|u|`` are masked, ordered by the
   bit pattern of ``|u|`` as an unsigned integer (numpy's order, NaN last).
   **Ties at the threshold: the lower index is masked first**
   (``np.argsort(kind="stable")``).  The reference's default ``argsort`` is
   unstable and breaks such ties arbitrarily; this rule is the one refinement.
3. ``mu = T(S / (n - mask_num))``, ``S`` the float64 sum of the survivors'
   ``|u|``; 0 when everything is masked.
4. ``sparse = mu * sign(u_masked)``; ``res = u - sparse``; ``acc += sparse``.

CUDA float32 / float64 tensors run the HIP kernels (``kernels.stc``, one
radix select per tensor, nothing leaves the device) and give device tensors.
numpy arrays and CPU tensors run a numpy implementation of the same
definition, which CPU parties use; so do integer entries of a state dict
(``num_batches_tracked``), computed in float64 as numpy would promote them.
Host and device add ``S`` in different orders, so their ``mu`` may differ in
the last bit; support and signs do not depend on that order.

Structure-wise pruning (SCR), the reference's ``SCRSparse``
(``sparse_compressor.py:182-230``) and the ``fed_scr`` worker's step around it
(``fed_scr.py:97-125``), is ``scr_step`` / ``SCRSparse`` at the end of this
file; its definition stands in ``scr_step``'s docstring.

The COO transport of what the two compressors produce (``sparse_encode`` /
``sparse_decode``, ``sparse_compressor.py:234-284``) lives in
``sfl_amd.utils.sparse`` and is re-exported here.

The quantized compressors for dense payloads (``QuantizedZeroPoint``,
``QuantizedLSTM``, ``QuantizedFP``, ``QuantizedKmeans``,
``quantized_compressor.py:65-279``) live in
``sfl_amd.utils.quantized`` and are re-exported here too.

``TopkSparse``, ``RandomSparse`` and ``MixedCompressor``
(``sparse_compressor.py:23-139``, ``mixed_compressor.py:23-111``), the two base
classes and the ``get(name, params)`` factory live in
``sfl_amd.utils.sparse_compressor`` and are re-exported here as well.
"""

from __future__ import annotations

from typing import List

import numpy as np
import torch

_KEY = {np.dtype(np.float32): (np.uint32, np.uint32(0x7FFFFFFF)),
        np.dtype(np.float64): (np.uint64, np.uint64(0x7FFFFFFFFFFFFFFF))}

_scratch: dict = {}


def mask_count(sparse_rate: float, n: int) -> int:
    """The reference's ``round(self.sparse_rate * weight_len)``."""
    return round(sparse_rate * n)


def _check_rate(sparse_rate: float) -> None:
    assert 0 <= sparse_rate <= 1, f"sparse rate should between 0 and 1, but get {sparse_rate}"


def _stc_numpy(u: np.ndarray, mask_num: int):
    """(sparse, mu) of flat float32 / float64 ``u``."""
    n, T = u.size, u.dtype.type
    kt, km = _KEY[u.dtype]
    key = u.view(kt) & km
    keep = np.ones(n, dtype=bool)
    keep[np.argsort(key, kind="stable")[:mask_num]] = False
    um = np.where(keep, u, T(0))
    mu = T(0) if mask_num == n else T(np.sum(np.abs(um), dtype=np.float64) / (n - mask_num))
    with np.errstate(invalid="ignore"):
        return mu * np.sign(um), mu


def _scratch_for(t: torch.Tensor, need_bytes: int) -> torch.Tensor:
    """The device's scratch for the current stream, grown on demand.  STC and
    SCR share it: calls on a stream are ordered."""
    from .. import kernels as K

    key = (t.device.index, K._stream(t))
    s = _scratch.get(key)
    if s is None or s.numel() < need_bytes:
        s = _scratch[key] = torch.empty(need_bytes, dtype=torch.uint8, device=t.device)
    return s


def _form_host(a, b, r) -> np.ndarray:
    """``u = (a - b) + r`` in numpy; an absent ``b`` or ``r`` is skipped."""
    u = np.asarray(a)
    if b is not None:
        u = np.subtract(u, np.asarray(b))
    if r is not None:
        u = np.add(u, np.asarray(r))
    return u


def _run_where_it_lives(who: str, device_fn, host_fn, a, b, r, acc=None):
    """One step on ``(a, b, r, acc)`` where ``a`` lives.  CUDA float32 /
    float64 tensors go to ``device_fn``; everything else goes to ``host_fn``
    as numpy arrays, and the first two results (``sparse``, ``res`` or None)
    come back as what ``a`` was: CUDA integer entries cross pinned memory both
    ways (``acc`` is written back), CPU tensors are viewed (``acc`` in place),
    numpy stays numpy.  Further results (``mu``) pass as ``host_fn`` gave them."""
    ops = (a, b, r, acc)
    if not isinstance(a, torch.Tensor):
        return host_fn(*ops)
    if a.is_cuda and a.dtype in (torch.float32, torch.float64):
        if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ops if t is not None):
            raise ValueError(f"{who}: every operand of a device step is a device tensor")
        return device_fn(*ops)
    if a.is_cuda:  # integer state entries: the numpy path, across pinned memory
        from .. import hostpipe as H

        host = [None if t is None else H.d2h(t, pooled=False) for t in ops]
        out = host_fn(*host)
        if acc is not None:
            acc.copy_(H.h2d(host[3], a.device))
        back = lambda x: H.h2d(x, a.device)  # noqa: E731
    else:
        out = host_fn(*(None if t is None else t.detach().numpy() for t in ops))  # views: acc in place
        back = torch.from_numpy
    return (*(None if x is None else back(x) for x in out[:2]), *out[2:])


def _stc_device(a, b, r, acc, sparse_rate):
    from .. import kernels as K

    shape = a.shape
    flat = [None if t is None else t.detach().contiguous().reshape(-1) for t in (a, b, r)]
    n = flat[0].numel()
    sparse = torch.empty(n, dtype=a.dtype, device=a.device)
    res = torch.empty(n, dtype=a.dtype, device=a.device)
    mu = torch.zeros((), dtype=a.dtype, device=a.device)
    if acc is not None and (acc.dtype != a.dtype or acc.shape != shape or not acc.is_contiguous()
                            or acc.device != a.device):
        raise ValueError("stc_step: acc is a contiguous tensor of the data's dtype, shape and device")
    if n:
        K.stc(flat[0], flat[1], flat[2], mask_count(sparse_rate, n), sparse, res,
              acc=None if acc is None else acc.detach().view(-1), mu_out=mu.view(1),
              scratch=_scratch_for(flat[0], K.stc_scratch_bytes(n, a.dtype)))
    return sparse.view(shape), res.view(shape), mu


def _stc_host(a, b, r, acc, sparse_rate):
    u = _form_host(a, b, r)
    if u.dtype not in _KEY:  # integer state entries: float64, as numpy's mean * sign promotes them
        u = u.astype(np.float64)
    shape = u.shape
    flat = np.ascontiguousarray(u).reshape(-1)
    sparse, mu = _stc_numpy(flat, mask_count(sparse_rate, flat.size))
    with np.errstate(invalid="ignore"):
        res = np.subtract(flat, sparse)
    sparse = sparse.reshape(shape)
    if acc is not None:
        if acc.dtype != sparse.dtype or acc.shape != shape:
            raise ValueError("stc_step: acc has the data's dtype and shape")
        np.add(acc, sparse, out=acc)
    return sparse, res.reshape(shape), mu


def stc_step(a, b, r, sparse_rate: float, acc=None):
    """``(sparse, res, mu)`` of ``u = (a - b) + r`` (``b``, ``r`` optional) at
    ``sparse_rate``; ``acc`` (optional) is updated in place with ``+= sparse``.
    A worker calls it with (new weights, old weights, residual), the server
    with (aggregated update, None, residual, acc=server weights).  CUDA
    float32 / float64 tensors give device tensors (``mu`` a 0-d device
    tensor: nothing is synchronised); numpy arrays give numpy arrays and CPU
    tensors CPU tensors, through the numpy implementation."""
    _check_rate(sparse_rate)
    return _run_where_it_lives("stc_step", lambda *ops: _stc_device(*ops, sparse_rate),
                               lambda *ops: _stc_host(*ops, sparse_rate), a, b, r, acc)


class STCSparse:
    """The reference's ``STCSparse``: callable on a list of arrays, gives the
    list of their ternary tensors (dense, the arrays' shapes)."""

    def __init__(self, sparse_rate: float):
        _check_rate(sparse_rate)
        self.sparse_rate = sparse_rate
        self.name = "STC"

    def __call__(self, weights: List) -> List:
        return [stc_step(w, None, None, self.sparse_rate)[0] for w in weights]


# ---------------------------------------------------------------------------
# structure-wise pruning (SCR)
# ---------------------------------------------------------------------------
def _view3(shape):
    """``[R, C, K]`` of a dense ``[R, C]`` or conv ``[O, I, H, W]`` layer; None: not pruned."""
    if len(shape) == 2:
        return int(shape[0]), int(shape[1]), 1
    if len(shape) == 4:
        return int(shape[0]), int(shape[1]), int(shape[2]) * int(shape[3])
    return None


def _scr_drops(mag: np.ndarray, threshold: float) -> np.ndarray:
    """Which structures go, from their float64 sums of magnitudes."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return mag / np.max(mag) <= np.float64(threshold)  # np.max propagates NaN; NaN compares false


def _scr_host(a, b, r, threshold, want_res):
    u = _form_host(a, b, r)
    sparse = np.array(u, copy=True, order="C")  # the inputs stay as they are
    v3 = _view3(u.shape)
    if v3 is not None and u.size:
        s3 = sparse.reshape(v3)
        mag = np.abs(s3)
        rows = _scr_drops(np.sum(mag, axis=(1, 2), dtype=np.float64), threshold)
        s3[rows] = 0
        cols = _scr_drops(np.sum(mag[~rows], axis=(0, 2), dtype=np.float64), threshold)
        s3[:, cols] = 0
    if not want_res:
        return sparse, None
    with np.errstate(invalid="ignore"):
        return sparse, np.subtract(u, sparse)


def _scr_device(a, b, r, threshold, want_res):
    from .. import kernels as K

    shape, v3 = a.shape, _view3(a.shape)
    if v3 is None:  # biases and the like: untouched
        u = a.detach()
        if b is not None:
            u = torch.sub(u, b)
        if r is not None:
            u = torch.add(u, r)
        u = u.clone() if u.data_ptr() == a.data_ptr() else u
        return u, (torch.sub(u, u) if want_res else None)
    flat = [None if t is None else t.detach().contiguous().reshape(-1) for t in (a, b, r)]
    sparse = torch.empty_like(flat[0])
    res = torch.empty_like(flat[0]) if want_res else None
    if sparse.numel():
        K.scr(flat[0], flat[1], flat[2], v3, threshold, sparse, res,
              scratch=_scratch_for(flat[0], K.scr_scratch_bytes(v3, a.dtype)))
    return sparse.view(shape), (res.view(shape) if want_res else None)


def scr_step(a, b, r, threshold: float, want_res: bool = True):
    """``(sparse, res)`` of ``u = (a - b) + r`` (``b``, ``r`` optional) pruned
    structure-wise at ``threshold``; ``res`` is None without ``want_res``.

    The definition, for a tensor of type T seen as ``[R, C, K]`` (a dense
    layer ``[R, C]`` with ``K = 1``, a conv layer ``[O, I, H, W]`` with
    ``K = H * W``; every other rank passes through untouched):

    1. ``u = (a - b) + r``, every operation rounded in T.
    2. ``S0[i]`` is the float64 sum of ``|u[i, :, :]|``; row ``i`` is dropped
       iff ``S0[i] / max(S0) <= threshold`` (float64; ``max`` propagates NaN).
    3. ``S1[j]`` is the float64 sum of ``|u[i, j, :]|`` over the kept rows;
       column ``j`` is dropped by the same rule.
    4. ``sparse`` is ``u`` with the dropped rows and columns ``+0.0`` (a kept
       element keeps its bits); ``res = u - sparse``.

    An all-zero tensor or one with a NaN drops nothing, a row with an inf is
    kept while the finite rows go (``threshold >= 0``), a negative threshold
    drops nothing: IEEE arithmetic, as in numpy.  **The one refinement against
    the reference (``SCRSparse``, sparse_compressor.py:182-230): the sums and
    ratios are float64, the reference's have the tensor's type.**  For
    float32 tensors the two differ only where a ratio lies within rounding
    (about 1e-6 relative) of the threshold.

    CUDA float32 / float64 tensors of rank 2 or 4 run the HIP kernels
    (``kernels.scr``; nothing leaves the device) and give device tensors;
    other ranks on the device use torch ops.  numpy arrays, CPU tensors and
    integer entries run numpy; integer results stay in their own dtype.  Host
    and device add the sums in different orders (about 1e-13 relative), which
    matters only for a ratio that close to the threshold."""
    return _run_where_it_lives("scr_step", lambda a, b, r, _: _scr_device(a, b, r, threshold, want_res),
                               lambda a, b, r, _: _scr_host(a, b, r, threshold, want_res), a, b, r)


class SCRSparse:
    """The reference's ``SCRSparse``: callable on a list of arrays, gives the
    list of their pruned tensors (dense, the arrays' shapes).

    It returns NEW arrays and leaves its inputs untouched.  The reference
    zeroes its inputs in place and returns the same objects, which is why its
    worker's residual ``dense - sparse`` (fed_scr.py:120-123) subtracts an
    array from itself and is identically zero."""

    def __init__(self, threshold: float):
        self.threshold = threshold
        self.name = "SCR"

    def __call__(self, weights: List) -> List:
        return [scr_step(w, None, None, self.threshold, want_res=False)[0] for w in weights]


from .sparse import SparseCOO, payload_nbytes, sparse_decode, sparse_encode  # noqa: E402,F401
from .quantized import (KmeansCompressData, QuantizedCompressedData, QuantizedCompressor, QuantizedFP,  # noqa: E402,F401
                        QuantizedKmeans, QuantizedLSTM, QuantizedZeroPoint)
from .sparse_compressor import (CompressedData, Compressor, MixedCompressedData, MixedCompressor,  # noqa: E402,F401
                                RandomSparse, SparseCompressedData, SparseCompressor, SparseMask, TopkSparse, get)
