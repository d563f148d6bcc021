"""What the robust plaintext aggregators share (``FlameAggregator``,
``MarsAggregator``, ``FreqAggregator``; each module's docstring is its
algorithm's definition): the surface towards ``FLModel``, the reading of the
uploads and weights, the move of mixed uploads onto one device, and the plain
weighted average of the kept clients that MARS and FreqFed end with.
"""

from __future__ import annotations

from typing import List, Sequence

import numpy as np
import torch

from ...device import PYU, DeviceObject
from .aggregator import Aggregator

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))
_TORCH_FLOATS = {torch.float32: _FLOATS[0], torch.float64: _FLOATS[1]}


# ------------------------------------------------------------- arguments
def _host(x):
    if isinstance(x, torch.Tensor):
        from ... import hostpipe as H

        return H.d2h(x, pooled=False) if x.is_cuda else x.detach().numpy()
    return np.asarray(x)


def _weights(weights, C: int) -> List[float]:
    if weights is None:
        return [1.0] * C
    if not isinstance(weights, (list, tuple)) or len(weights) != C:
        raise ValueError(f"weights: one scalar per client ({C}) or None")
    out = []
    for i, v in enumerate(weights):
        v = _host(v)  # (a device scalar: through a pinned buffer)
        if v.ndim != 0 or v.dtype.kind not in "fiub":
            raise ValueError(f"weights: client {i}'s weight is not one number (per-element weights are not FLAME's)")
        if not np.isfinite(v):
            raise ValueError(f"weights: client {i}'s weight is not finite")
        out.append(float(v))
    return out


def _np_dtype(x):
    """The numpy type of a layer; a tensor of a type the aggregators do not take keeps its
    torch type, which equals no numpy type (None would: numpy reads it as float64)."""
    return _TORCH_FLOATS.get(x.dtype, x.dtype) if isinstance(x, torch.Tensor) else np.dtype(x.dtype)


def _layers(data: list) -> list:
    """``data[i][l]`` -> ``layers[l][i]``, with one shape and one float type per layer."""
    L0 = len(data[0])
    for i, d in enumerate(data):
        if len(d) != L0:
            raise ValueError(f"client {i} uploads {len(d)} layers, client 0 uploads {L0}")
    layers = [[d[l] for d in data] for l in range(L0)]
    for l, xs in enumerate(layers):
        shape, dtype = tuple(xs[0].shape), _np_dtype(xs[0])
        if dtype not in _FLOATS:
            raise ValueError(f"layer {l}, client 0: float32 or float64, not {xs[0].dtype}")
        for i, x in enumerate(xs):
            if tuple(x.shape) != shape or _np_dtype(x) != dtype:
                raise ValueError(f"layer {l}, client {i}: shape {tuple(x.shape)} and type {x.dtype} differ from "
                                 f"client 0's {shape} and {xs[0].dtype}")
    return layers


def _one_type(layers: list) -> None:
    for l, xs in enumerate(layers):
        if _np_dtype(xs[0]) != _np_dtype(layers[0][0]):
            raise ValueError(f"layer {l}, client 0: type {xs[0].dtype} differs from layer 0's {layers[0][0].dtype}")


# ---------------------------------------------------------- the device path
def upload(layers: list, dev, who: str, limit: int = 16, macro: str = "SA_FLAME_MAX_CLIENTS") -> list:
    """``layers[l][i]`` as flat contiguous tensors on ``dev``: at most
    ``limit`` clients (the library's ``macro``); a host layer among device ones
    goes there through pinned memory."""
    from ... import hostpipe as H

    C = len(layers[0])
    if C > limit:
        raise NotImplementedError(f"{who} takes at most {limit} clients on the device ({macro}), got {C}; the host "
                                  f"form takes any number")
    on_dev = []
    for l, xs in enumerate(layers):
        row = []
        for i, x in enumerate(xs):
            if isinstance(x, torch.Tensor) and x.is_cuda:
                if x.device != dev:
                    raise ValueError(f"layer {l}, client {i}: on {x.device}, the others on {dev}")
                row.append(x.detach().contiguous().reshape(-1))
            else:  # a host layer among device ones: through pinned memory
                row.append(H.h2d(x, dev).reshape(-1))
        on_dev.append(row)
    return on_dev


def average_host(xs: Sequence[np.ndarray], w: Sequence[float]) -> np.ndarray:
    """MARS's and FreqFed's last step for one layer over the kept clients' arrays."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.average(xs, axis=0, weights=w) + 0.0


def average_kept(layers: list, on_dev: list, w: List[float], keep: List[bool], dev) -> list:
    """``average_host`` on the device over ``upload``'s tensors (``sa_flame_combine`` with a zero median and unit
    scales): float64 layers in the uploads' shapes."""
    from ... import hostpipe as H
    from ... import kernels as K

    C = len(layers[0])
    kept_w = [w[i] for i in range(C) if keep[i]]
    W = float(np.asarray(kept_w, np.float64).sum())
    if W == 0.0:
        raise ZeroDivisionError("Weights sum to zero, can't be normalized")
    zero = torch.zeros(max(row[0].numel() for row in on_dev), dtype=on_dev[0][0].dtype, device=dev)
    outs = []
    for xs, row in zip(layers, on_dev):
        n = row[0].numel()
        if n <= 1:  # np.average itself (flame_aggregator's step 4), on a copy of at most one element
            host = average_host([H.d2h(row[i], pooled=False) for i in range(C) if keep[i]], kept_w)
            outs.append(H.h2d(host, dev).reshape(tuple(xs[0].shape)))
            continue
        out = torch.empty(n, dtype=torch.float64, device=dev)
        K.flame_combine(row, [1.0] * C, w, keep, zero[:n], W, out)
        outs.append(out.reshape(tuple(xs[0].shape)))
    return outs


# ------------------------------------------------------------------ the surface
class RobustAggregator(Aggregator):
    """A plaintext aggregator whose ``average`` leaves suspected clients out:
    every party's update reaches the server in the clear.  A subclass defines
    ``_average(parties, weights)`` on the server; ``last_report`` holds what its
    last call decided."""

    def __init__(self, device: PYU):
        assert isinstance(device, PYU), f"Accepts PYU only but got {type(device)}."
        self.device = device
        self.last_report = None

    def _parse(self, parties: list, weights, one_type: bool = False) -> tuple:
        """What every ``_average`` starts from: whether the parties sent one layer
        and not a list, ``data[i][l]`` as arrays and tensors, ``layers[l][i]``, a
        float weight per client, and the device of the first CUDA layer or None."""
        single = not isinstance(parties[0], (list, tuple))
        data = [[p] if single else list(p) for p in parties]
        data = [[x if isinstance(x, torch.Tensor) else np.asarray(x) for x in d] for d in data]
        for i, d in enumerate(data):
            for l, x in enumerate(d):
                if type(x).__name__ == "SparseCOO" or x.dtype == object:
                    raise ValueError(f"layer {l}, client {i}: {type(self).__name__} takes dense float layers (sparse "
                                     f"uploads: SparsePlainAggregator)")
        w = _weights(weights, len(data))
        layers = _layers(data)
        if one_type:
            _one_type(layers)
        dev = next((x.device for xs in layers for x in xs if isinstance(x, torch.Tensor) and x.is_cuda), None)
        return single, data, layers, w, dev

    def _run(self, data: List[DeviceObject], fn):
        assert data, "Data to aggregate should not be None or empty!"
        data = [d.to(self.device) for d in data]
        return self.device(fn)(*data)

    def sum(self, data: List[DeviceObject], axis=None) -> DeviceObject:
        """Sum of array elements over a given axis (the reference inherits
        ``PlainAggregator.sum`` unchanged: ``np.sum`` over the stacked parties,
        per layer for per-layer lists).  Device float64 layers summed over the
        parties stay on the device (``kernels.sum_f64``); other device layers
        are read to the host."""
        def one(xs):
            if axis == 0 and all(isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float64 for x in xs) \
                    and all(x.shape == xs[0].shape and x.device == xs[0].device for x in xs):
                from ... import kernels as K

                return K.sum_f64([x.detach().contiguous() for x in xs], torch.empty_like(xs[0].contiguous()))
            return np.sum([_host(x) for x in xs], axis=axis)

        def _sum(*parties):
            if isinstance(parties[0], (list, tuple)):
                return [one(list(layer)) for layer in zip(*parties)]
            return one(list(parties))

        return self._run(data, _sum)

    def average(self, data: List[DeviceObject], axis=None, weights=None) -> DeviceObject:
        """The robust average over the parties (the subclass's module has the definition)."""
        if axis not in (None, 0):
            raise ValueError(f"{type(self).__name__} aggregates over the parties (axis 0 or None), not axis {axis}")
        if isinstance(weights, (list, tuple)):
            weights = [wt.to(self.device).data if isinstance(wt, DeviceObject) else wt for wt in weights]
        return self._run(data, lambda *parties: self._average(list(parties), weights))
