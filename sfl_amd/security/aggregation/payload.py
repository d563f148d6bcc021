"""What a secure-aggregation payload is: its layers and container, the
element type a layer is shipped to the GPU as and the arithmetic type
``datum * weight`` is quantized in, its weight on the host, its flat host
form and its device form.  Both drivers -- the in-process
``secure_aggregator.SecureAggregator`` and the per-party functions of
``party`` -- plan their launches from here.

Imports without torch (a party process may not have it at import time); the
functions that need it import it on use.
"""

from __future__ import annotations

import functools
import sys

import numpy as np

F32, F64, I64 = np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.int64)

# per-party bytes up to which a call is latency-bound (tools/config1_bench.py
# at 9 .. 1M elements): host arrays packed into one pinned copy and host
# results collected after one synchronisation; above it the driver's pageable
# copies, which pipeline their staging, are faster than a host memcpy
# into pinned memory
SMALL_CALL_BYTES = 1 << 20


@functools.lru_cache(maxsize=None)
def torch_dtypes() -> dict:
    """The three element / arithmetic types as torch dtypes (torch is imported on first use)."""
    import torch

    return {F32: torch.float32, F64: torch.float64, I64: torch.int64}


def is_torch(a) -> bool:
    torch = sys.modules.get("torch")  # a tensor exists only where torch is loaded (and no import per call)
    return torch is not None and isinstance(a, torch.Tensor)


def np_dtype(a) -> np.dtype:
    """The numpy dtype of a layer: an array's own, a torch tensor's by name, else what ``np.asarray`` gives."""
    dt = getattr(a, "dtype", None)
    if isinstance(dt, np.dtype):
        return dt
    return np.asarray(a).dtype if dt is None else np.dtype(str(dt).replace("torch.", ""))


def shape(a):
    return tuple(a.shape) if hasattr(a, "shape") else np.shape(a)


def compute_dtype(ldt: np.dtype, w, fxp_bits: int) -> np.dtype:
    """Result dtype of ``(datum * w) * (1 << fxp)`` under the numpy the
    reference pins, 1.23.5 (``uv.lock:1189-1190``): value-based casting, so a
    scalar weight -- python OR numpy scalar / 0-d array -- does not widen
    the array's dtype when its value fits (``result_type(dtype,
    min_scalar_type(w))``); array weights promote as usual.  numpy 2's NEP 50
    would make a numpy-scalar weight "strong" (float32 data * np.float64(w)
    -> float64); no reference fixture pins either (parity
    unpinned), the pinned version decides.  Python scalars behave alike
    under both rules."""
    if w is None:
        return _unweighted_dtype(ldt, fxp_bits)
    probe = np.zeros(1, dtype=ldt)
    if isinstance(w, (bool, int, float)) and not isinstance(w, np.generic):  # np.float64 is a float
        probe = probe * w
    else:
        wa = np.asarray(w)
        dt = np.result_type(ldt, wa.dtype if wa.ndim else np.min_scalar_type(wa))
        probe = probe.astype(dt)
    return (probe * (1 << fxp_bits)).dtype


@functools.lru_cache(maxsize=None)
def _unweighted_dtype(ldt: np.dtype, fxp_bits: int) -> np.dtype:
    """``compute_dtype`` without a weight, kept per dtype: every unweighted
    small call asks for it, and a small call counts microseconds."""
    return (np.zeros(1, dtype=ldt) * (1 << fxp_bits)).dtype


def element_types(ldt: np.dtype, w, fxp_bits: int) -> tuple:
    """(element type, arithmetic type) of a layer of dtype ``ldt`` under
    weight ``w``: the data go to the GPU as float32 / float64 / int64 (other
    integers and bools widened to int64, other floats to float64) and
    ``datum * w`` is quantized in ``compute_dtype``."""
    ct = compute_dtype(ldt, w, fxp_bits)
    if ct not in (F32, F64, I64):
        raise NotImplementedError(f"arithmetic type {ct} (data {ldt}) is not supported")
    if ldt.kind in "biu" and ldt != I64 and ct.kind == "i":
        raise NotImplementedError(f"integer data of type {ldt} is not supported")
    xt = ldt if ldt in (F32, F64, I64) else (I64 if ldt.kind in "biu" else F64)
    return xt, ct


def scalar_weight(w, ct: np.dtype):
    """A scalar weight in the arithmetic's kind (float, or int for int64)."""
    return float(w) if ct.kind == "f" else int(w)


def host_weight(w):
    """A weight as the host sees it: a torch tensor becomes its numpy array."""
    if is_torch(w):
        from ... import hostpipe as H

        return w.detach().numpy() if w.device.type == "cpu" else H.d2h(w, pooled=False)
    return w


def split_layers(payload) -> tuple:
    """(layers, container) of a party's payload; ``container`` is "array" |
    "list" | "tuple", as ``party.MaskedPayload`` names them."""
    if isinstance(payload, tuple):
        return list(payload), "tuple"
    if isinstance(payload, list):
        return list(payload), "list"
    return [payload], "array"


def flat_host(layers, dtype=None, out=None) -> np.ndarray:
    """The layers' elements as one flat host vector: a view of a single
    layer that already has ``dtype``, else a packed copy -- into ``out`` (a
    row of pinned memory) when given."""
    if len(layers) == 1 and out is None:
        return np.asarray(layers[0], dtype=dtype).reshape(-1)
    return np.concatenate([np.asarray(a, dtype=dtype).reshape(-1) for a in layers], out=out)


def to_device(a, xt: np.dtype, dev):
    """One layer as a flat, contiguous, 16-byte aligned ``xt`` tensor on the
    torch device ``dev``."""
    from ... import hostpipe as H

    tdt = torch_dtypes()[xt]
    if is_torch(a) and a.device.type != "cpu":
        t = a.detach().reshape(-1).to(device=dev, dtype=tdt)
    elif is_torch(a):  # cast on the host (no DMA), then a pinned copy
        t = H.h2d(a.detach().reshape(-1).to(tdt), dev)
    else:
        t = H.h2d(np.ascontiguousarray(np.asarray(a), dtype=xt).reshape(-1), dev)
    t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t
