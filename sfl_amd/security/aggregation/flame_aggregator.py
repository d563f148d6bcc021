"""The robust plaintext aggregator, mirroring the reference's FLAME
aggregator (``examples/security/h_bd/agg_flame.py:27-203``, the
``aggregator=`` of ``backdoor_fl_torch.py``): outliers among the clients are
left out, the others' updates are clipped to the median update norm and
averaged.

The definition (``C`` clients in list order, each a list of ``L`` layers of
one float type ``T``, float32 or float64; ``flame_host`` below is the same
text as code, and the device path computes the same numbers with
``sa_flame_stats`` / ``sa_flame_combine``, include/sfl_sa.h):

1. **Median.**  For every layer and element ``g`` = the median of the ``C``
   values in ``T``: the middle one for odd ``C``, ``(lo + hi) / T(2)`` for
   even ``C`` with the add and the divide each rounded in ``T`` (the add may
   overflow to ``inf``, as numpy's).  A NaN among the values gives NaN.  The
   order is the total order of the bit patterns with ``-0 < +0``: a tie of
   zeros is decided, where numpy's partition leaves it arbitrary.  Without
   such ties this is ``np.median(np.stack(...), axis=0)`` bit for bit.
2. **Statistics**, float64, over all layers of a client as one flat vector:
   ``G[i][j] = sum x_i x_j`` over the raw parameters (operands converted to
   float64 first) and ``N[i] = sum d_i^2`` with ``d_i = x_i - g`` rounded in
   ``T`` (the reference's ``arr - estimated_global``), squared in float64.
   The order of summation belongs to the implementation (numpy's pairwise
   sums here, the kernel's fixed wave order on the device); layers are added
   in layer order.
3. **Decisions** (``decide``; host code over ``C (C + 1) / 2 + C`` doubles,
   shared by both paths).  A non-finite statistic raises ``ValueError`` naming
   the client (the reference's ``cosine_distances`` raises on NaN and inf
   too).  ``cd[i][j] = clip(1 - G[i][j] / sqrt(G[i][i] G[j][j]), 0, 2)``, 0 on
   the diagonal; a client with ``G[i][i] == 0`` is at distance 1 from every
   other, as sklearn's ``normalize`` has it.  **Inliers**: with
   ``m = int(C / 2 + 1)``, the smallest ``t`` for which the graph
   ``{cd[i][j] <= t}`` has a connected component of at least ``m`` clients;
   that component (unique, since ``m > C / 2``) gets label 0, everyone else
   -1.  This is what the reference's ``HDBSCAN(min_cluster_size=m,
   min_samples=1, allow_single_cluster=True, metric="precomputed")`` computes,
   without the library: with ``min_samples=1`` the mutual-reachability
   distance is the distance itself, the condensed tree is single linkage and
   no true split can exist (two clusters of ``m`` clients each would need
   ``2 m > C`` clients).  At least ``m`` clients are always kept, so the
   reference's fallback for "every client filtered" (``agg_flame.py:174-175``)
   is unreachable and is not built.  ``norm_i = sqrt(N[i])``,
   ``threshold = np.median(norms)``, ``scale_i = min(1, threshold / norm_i)``
   if ``norm_i > 0`` else 1: float64 from float64 sums, where the reference
   takes float32 ``np.linalg.norm``s whose bits depend on the BLAS.
4. **Combine.**  Per element, over the inliers in client order, with
   ``s_i = T(scale_i)``: ``m_i = g + (x_i - g) * s_i``, every operation
   rounded in ``T``, nothing contracted; ``acc = acc + float64(m_i) *
   float64(w_i)`` from ``+0.0``, multiply and add rounded separately;
   ``out = acc / W + 0.0`` with ``W = np.asarray(w_inliers, float64).sum()``.
   The ``+ 0.0`` is the reference's zero-variance noise term (``lamda = 0``,
   ``agg_flame.py:194-199``): it turns ``-0`` into ``+0``.  A non-zero noise
   multiplier is not built.  This equals the reference's steps 5 to 8
   (``np.average(..., weights=) + noise``) bit for bit; a layer of at most one
   element goes through ``np.average`` itself, because numpy reduces those
   pairwise (``SparsePlainAggregator`` makes the same exception).

Weights are one finite scalar per client (``None``: 1.0 each); anything else
raises ``ValueError``.  The result is a list of float64 layers.
"""

from __future__ import annotations

import logging
from typing import List, Sequence

import numpy as np
import torch

from ...device import PYU, DeviceObject
from .aggregator import Aggregator

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))
MAX_DEVICE_CLIENTS = 16  # SA_FLAME_MAX_CLIENTS: the kernels' client count is a template argument

log = logging.getLogger(__name__)


# ------------------------------------------------------------------ the median
def median_host(stack: np.ndarray) -> np.ndarray:
    """Step 1 over ``stack`` of shape ``(C, ...)``: the median along axis 0 in
    the stack's own float type, by the order of the bit patterns."""
    T = stack.dtype
    if T not in _FLOATS:
        raise ValueError(f"float32 or float64, not {T}")
    I = np.int32 if T == np.float32 else np.int64
    bits, mag = 8 * T.itemsize - 1, I(np.iinfo(I).max)
    b = np.ascontiguousarray(stack).view(I)
    keys = np.sort(b ^ ((b >> bits) & mag), axis=0)  # negative patterns: magnitude bits flipped
    C = stack.shape[0]

    def value(k):
        return np.ascontiguousarray(k ^ ((k >> bits) & mag)).view(T)

    if C % 2:
        g = value(keys[C // 2])
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            g = (value(keys[C // 2 - 1]) + value(keys[C // 2])) / T.type(2)
    return np.where(np.isnan(stack).any(axis=0), T.type(np.nan), g).astype(T, copy=False)


# --------------------------------------------------------------- the statistics
def stat_count(C: int) -> int:
    return C * (C + 1) // 2 + C


def stats_host(layers: Sequence[Sequence[np.ndarray]], medians: Sequence[np.ndarray]) -> np.ndarray:
    """Step 2: ``layers[l][i]`` is client ``i``'s layer ``l``; the packed upper
    triangle of ``G`` (row-major, ``j >= i``), then ``N``."""
    C = len(layers[0]) if layers else 0
    out = np.zeros(stat_count(C), np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for xs, g in zip(layers, medians):
            x64 = [np.asarray(x, np.float64).reshape(-1) for x in xs]
            s = 0
            for i in range(C):
                for j in range(i, C):
                    out[s] += np.sum(x64[i] * x64[j], dtype=np.float64)
                    s += 1
            for i in range(C):
                d = (xs[i] - g).astype(np.float64).reshape(-1)  # the difference rounds in T
                out[s + i] += np.sum(d * d, dtype=np.float64)
    return out


# ----------------------------------------------------------------- the decisions
def inliers(cd: np.ndarray) -> List[int]:
    """Label 0 for the first connected component of at least ``int(C / 2 + 1)``
    clients as the distance threshold grows, -1 for everyone else: a union-find
    over the sorted edges, all edges of one distance admitted together."""
    C = len(cd)
    m = int(C / 2 + 1)
    parent, size = list(range(C)), [1] * C

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    edges = sorted((float(cd[i][j]), i, j) for i in range(C) for j in range(i + 1, C))
    at, root = 0, 0 if m <= 1 else None
    while root is None:
        t = edges[at][0]
        while at < len(edges) and edges[at][0] == t:
            a, b = find(edges[at][1]), find(edges[at][2])
            if a != b:
                a, b = (a, b) if size[a] >= size[b] else (b, a)
                parent[b], size[a] = a, size[a] + size[b]
            at += 1
        root = next((r for r in range(C) if parent[r] == r and size[r] >= m), None)
    return [0 if find(i) == root else -1 for i in range(C)]


def decide(stats, C: int) -> dict:
    """Step 3 from the ``stat_count(C)`` statistics, wherever they were
    computed: labels, norms, threshold, scales and the cosine distances."""
    stats = np.asarray(stats, np.float64).reshape(-1)
    if stats.size != stat_count(C):
        raise ValueError(f"{stat_count(C)} statistics expected for {C} clients, got {stats.size}")
    G = np.zeros((C, C), np.float64)
    G[np.triu_indices(C)] = stats[:C * (C + 1) // 2]
    N = stats[C * (C + 1) // 2:]
    # a client's own squared norm first: its NaN spreads into every median and every other statistic
    for ok in (np.isfinite(np.diag(G)), np.isfinite(N), np.isfinite(G).all(axis=1)):
        if not ok.all():
            raise ValueError(f"client {int(np.argmin(ok))}: non-finite parameters (a NaN, an infinity or an "
                             f"overflowing sum): FLAME's cosine distances and norms are undefined")
    cd = np.zeros((C, C), np.float64)
    for i in range(C):
        for j in range(i + 1, C):
            if G[i, i] == 0.0 or G[j, j] == 0.0:
                d = 1.0
            else:
                with np.errstate(over="ignore"):
                    d = 1.0 - G[i, j] / np.sqrt(G[i, i] * G[j, j])
                if not np.isfinite(d):
                    raise ValueError(f"client {i}: the squared norms' product overflows float64")
            cd[i, j] = cd[j, i] = min(max(d, 0.0), 2.0)
    norms = np.sqrt(N)
    threshold = np.median(norms)
    scales = np.array([min(1.0, threshold / v) if v > 0 else 1.0 for v in norms], np.float64)
    return {"labels": inliers(cd), "norms": norms, "threshold": float(threshold), "scales": scales,
            "cosine_distances": cd}


# ------------------------------------------------------------------- the combine
def combine_host(xs: Sequence[np.ndarray], g: np.ndarray, scales, weights, keep) -> np.ndarray:
    """Step 4 for one layer: ``xs`` the clients' arrays of type ``T``, ``g``
    their median, one scale, weight and keep flag per client."""
    T = g.dtype
    kept = [i for i in range(len(xs)) if keep[i]]
    w = [float(weights[i]) for i in kept]
    W = np.asarray(w, np.float64).sum()
    if W == 0.0:
        raise ZeroDivisionError("Weights sum to zero, can't be normalized")
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        models = [g + (xs[i] - g) * T.type(scales[i]) for i in kept]
        if g.size <= 1:  # numpy reduces these pairwise: np.average itself
            return np.average(models, axis=0, weights=w) + 0.0
        acc = np.zeros(g.shape, np.float64)
        for m, wi in zip(models, w):
            acc = acc + m.astype(np.float64) * np.float64(wi)
        return acc / W + 0.0


def flame_host(data: Sequence[Sequence[np.ndarray]], weights=None) -> tuple:
    """The whole definition on host arrays: ``data[i][l]`` is client ``i``'s
    layer ``l``.  Returns (the float64 layers, the report)."""
    C = len(data)
    layers = _layers([[np.asarray(x) for x in d] for d in data])
    w = _weights(weights, C)
    medians = [median_host(np.stack(xs)) for xs in layers]
    report = decide(stats_host(layers, medians), C)
    keep = [lb == 0 for lb in report["labels"]]
    return [combine_host(xs, g, report["scales"], w, keep) for xs, g in zip(layers, medians)], report


# ------------------------------------------------------------- arguments
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


_TORCH_FLOATS = {torch.float32: _FLOATS[0], torch.float64: _FLOATS[1]}


def _np_dtype(x):
    """The numpy type of a layer; a tensor of a type FLAME does not take keeps its
    torch type, which equals no numpy type (None would: numpy reads it as float64)."""
    return _TORCH_FLOATS.get(x.dtype, x.dtype) if isinstance(x, torch.Tensor) else np.dtype(x.dtype)


class FlameAggregator(Aggregator):
    """FLAME aggregator (Byzantine-robust aggregation).

    The computation is performed in plaintext: every party's update reaches
    the server in the clear.  ``average`` over the parties runs the module's
    definition; when any layer of the uploads is a CUDA tensor the whole model
    is aggregated on that device (host layers among them go there through
    pinned memory) by ``sa_flame_stats`` and ``sa_flame_combine``, with one
    pinned read of the statistics between them, and the result is a list of
    float64 tensors on the device.  Uploads that are all host arrays run the
    numpy form and give float64 arrays.  The device path takes at most 16
    clients; the host form any number.

    After each ``average``, ``last_report`` holds ``labels`` (0 an inlier, -1
    left out), ``norms``, ``threshold``, ``scales`` and ``cosine_distances``.

    Sparse (COO) uploads are refused: ``FLModel(sparse_transport="both")``
    asks for ``accepts_sparse``, which this class does not declare.

    Examples:
      >>> aggregator = FlameAggregator(server)
      >>> fl = FLModel(server=server, device_list=clients, model=build, aggregator=aggregator)
    """

    def __init__(self, device: PYU):
        assert isinstance(device, PYU), f"Accepts PYU only but got {type(device)}."
        self.device = device
        self.last_report = None

    # ------------------------------------------------------------ the paths
    def _device_average(self, layers: list, w: List[float], dev) -> list:
        from ... import hostpipe as H
        from ... import kernels as K

        C = len(layers[0])
        if C > MAX_DEVICE_CLIENTS:
            raise NotImplementedError(f"FlameAggregator takes at most {MAX_DEVICE_CLIENTS} clients on the device "
                                      f"(SA_FLAME_MAX_CLIENTS), got {C}; the host form takes any number")
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
        stats = torch.zeros(K.flame_stat_count(C), dtype=torch.float64, device=dev)
        need = max(K.flame_scratch_bytes(r[0].numel(), C, r[0].dtype) for r in on_dev)
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        medians = []
        for l, row in enumerate(on_dev):
            g = torch.empty_like(row[0])
            K.flame_stats(row, g, scratch, stats, accumulate=l > 0)
            medians.append(g)
        report = decide(H.d2h(stats, pooled=False), C)  # the one read between the two passes
        keep = [lb == 0 for lb in report["labels"]]
        W = float(np.asarray([w[i] for i in range(C) if keep[i]], np.float64).sum())
        if W == 0.0:
            raise ZeroDivisionError("Weights sum to zero, can't be normalized")
        outs = []
        for xs, row, g in zip(layers, on_dev, medians):
            if g.numel() <= 1:  # np.average itself (the module's step 4), on a copy of at most one element
                host = combine_host([H.d2h(x, pooled=False) for x in row], H.d2h(g, pooled=False), report["scales"], w,
                                    keep)
                outs.append(H.h2d(host, dev).reshape(tuple(xs[0].shape)))
                continue
            out = torch.empty(g.numel(), dtype=torch.float64, device=dev)
            K.flame_combine(row, report["scales"], w, keep, g, W, out)
            outs.append(out.reshape(tuple(xs[0].shape)))
        self.last_report = report
        return outs

    def _average(self, parties: list, weights):
        single = not isinstance(parties[0], (list, tuple))
        data = [[p] if single else list(p) for p in parties]
        data = [[x if isinstance(x, torch.Tensor) else np.asarray(x) for x in d] for d in data]
        for i, d in enumerate(data):
            for l, x in enumerate(d):
                if type(x).__name__ == "SparseCOO" or x.dtype == object:
                    raise ValueError(f"layer {l}, client {i}: FlameAggregator takes dense float layers (sparse "
                                     f"uploads: SparsePlainAggregator)")
        C = len(data)
        w = _weights(weights, C)
        layers = _layers(data)
        dev = next((x.device for xs in layers for x in xs if isinstance(x, torch.Tensor) and x.is_cuda), None)
        if dev is not None:
            outs = self._device_average(layers, w, dev)
        else:
            host = [[x.detach().numpy() if isinstance(x, torch.Tensor) else x for x in xs] for xs in layers]
            medians = [median_host(np.stack(xs)) for xs in host]
            report = decide(stats_host(host, medians), C)
            keep = [lb == 0 for lb in report["labels"]]
            outs = [combine_host(xs, g, report["scales"], w, keep) for xs, g in zip(host, medians)]
            self.last_report = report
        log.info("Cluster labels: %s", self.last_report["labels"])
        return outs[0] if single else outs

    # --------------------------------------------------------------- surface
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
        """The robust average over the parties (the module's definition)."""
        if axis not in (None, 0):
            raise ValueError(f"FlameAggregator aggregates over the parties (axis 0 or None), not axis {axis}")
        if isinstance(weights, (list, tuple)):
            weights = [wt.to(self.device).data if isinstance(wt, DeviceObject) else wt for wt in weights]
        return self._run(data, lambda *parties: self._average(list(parties), weights))


def _host(x):
    if isinstance(x, torch.Tensor):
        from ... import hostpipe as H

        return H.d2h(x, pooled=False) if x.is_cuda else x.detach().numpy()
    return np.asarray(x)
