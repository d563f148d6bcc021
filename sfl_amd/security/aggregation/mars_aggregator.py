"""The Lipschitz-based robust plaintext aggregator, mirroring the reference's
MARS aggregator (``examples/security/h_bd/agg_mars.py:27-334``): every
client's model is summarised by the largest Lipschitz constants of its
channels (``CLP``), the clients are split in two by the shape of those
summaries, and one of the two groups is left out of the average when the
groups are far enough apart.

The definition (``C`` clients in list order, each a list of layers of one
float type ``T``, float32 or float64, with the same shapes in every client;
``mars_host`` below is the same text as code, and the device path computes the
features with ``sa_mars_sigma`` / ``sa_mars_bn``, include/sfl_sa.h):

1. **Plan** (``clp_plan``; ``agg_mars.py:46-71``).  A function of the layers'
   ``ndim`` only, walking the list from the front: a 4-D layer is a ``conv``;
   a 1-D layer with at least three more layers after it, all four 1-D, is a
   ``bn`` group of four (weight, bias, mean, variance) and the walk jumps by
   four; a 2-D layer is an ``fc``; anything else is skipped.  A ``conv`` takes
   its BatchNorm from the *next plan entry* if that entry is a ``bn``
   (``:80-85``: the weight at its index, the variance three further).  This is
   the reference's literal behaviour and it is kept, also where it misreads a
   model: a conv *bias* in front of a BatchNorm starts the group of four, so
   the "weight" is the conv bias and the "variance" the BatchNorm's running
   mean, and the BatchNorm's own variance, left over, is skipped.
2. **Features** (``features_host``), all float64.  ``sigma(W)`` is the largest
   singular value of ``W`` converted to float64.
   ``scale[ch] = |float64(bn_w[ch])| / sqrt(max(float64(bn_var[ch]), 0) + 1e-5)``.
   A conv channel: ``sigma(W[ch].reshape(C_in, kh * kw)) * scale[ch]`` when a
   ``bn`` follows and ``ch < len(bn_w)``, else ``sigma`` alone.  A bn channel:
   ``scale[ch]``.  An fc layer: ``sigma(W)``.  *Refinement*: the reference
   multiplies the float32 weights by the float32 scale before a float32
   LAPACK SVD, whose bits depend on the BLAS; here the scalar scale is applied
   once to a float64 ``sigma``.  The two agree mathematically and differ by
   float32 roundings.  A non-finite feature raises ``ValueError`` naming the
   client (the reference catches the failure and goes on with an empty
   vector).
3. **Decisions** (``decide``; host code over the features, shared by both
   paths; ``agg_mars.py:108-142`` and ``:161-247`` literally).  Per plan entry
   the features ``>= np.quantile(., 0.95)`` are kept, in plan order; with an
   empty plan the client's vector is the float64 norms of all its layers
   (``:145-152``).  Every vector becomes a 50-bin ``density=True`` histogram
   over its own range; ``D[i][j]`` is scipy's ``wasserstein_distance`` of two
   histograms; ``KMeans(n_clusters=2, random_state=42, n_init=10)`` runs on the
   rows of ``D``; a cluster's centre is the histogram of its members' vectors
   concatenated; when the two centres are farther apart (the same distance)
   than ``anomaly_threshold``, the cluster whose centre has the larger L1 norm
   gets label -1, everyone else 0.  Fewer than two clients, one empty cluster
   or centres within the threshold: every label is 0.  The reference's catch
   of a failed clustering ("every label 0") cannot be reached with finite
   features and is not built.
4. **Combine.**  ``np.average(layer_values, axis=0, weights=w_kept) + 0.0``
   over the kept clients in client order: float64 layers.  The ``+ 0.0``
   (``-0`` becomes ``+0``) is what the device's combine entry does
   (``sa_flame_combine`` with a zero median and unit scales computes
   ``0 + (x - 0) * 1 = x`` in ``T``, accumulates ``float64(x) * w`` in client
   order from ``+0.0`` and divides by ``W``: ``np.average`` bit for bit, see
   ``flame_aggregator``'s step 4, with the same exception for layers of at
   most one element).  If every client is dropped, client 0's upload is
   returned as it is (``:311-315``).  The reference's median fallback for a
   failed ``np.average`` cannot be reached with validated inputs and is not
   built.

Consequences worth knowing.  The histograms are densities over each vector's
*own* range, so a client whose largest constants are spread widely has a low
histogram: in the planted case of the tests (six clients, clients 1 and 4 with
a few channels scaled up by 4 to 8) the scaled-up pair is the cluster with the
*smaller* centre norm, and the four honest clients are dropped: labels
``[-1, 0, -1, -1, 0, -1]`` for thresholds 1.0, 0.1 and 0.01.  That is the
reference's behaviour, reproduced here.

Weights are one finite scalar per client (``None``: 1.0 each).  On the device
a layer whose smaller side exceeds ``SA_MARS_MAX_P`` (32), such as a hidden fc
layer, is read to the host and takes ``np.linalg.svd`` there
(``last_report["host_layers"]`` counts them) -- or, with
``wide_layers="device"``, stays on the device up to a smaller side of
``SA_MARS_WIDE_MAX_P`` (512) and takes ``sa_mars_sigma_wide`` (a tiled float64
Gram matrix, Householder reduction and Sturm counts;
``last_report["wide_layers"]`` counts them, and only what is beyond that limit
still goes to the host).  At most 16 clients are taken on the device; the host
form takes any number.
"""

from __future__ import annotations

import logging
from typing import List, Sequence

import numpy as np
import torch

from ...device import PYU
from .robust import RobustAggregator, _host, _layers, _one_type, _weights, average_host, average_kept, upload

MAX_P = 32  # SA_MARS_MAX_P: the Gram matrix of the smaller side lives in one wave's LDS
WIDE_MAX_P = 512  # SA_MARS_WIDE_MAX_P: the Gram matrix in scratch, one block a matrix
EPS = 1e-5
TOP = 0.05

log = logging.getLogger(__name__)


# ------------------------------------------------------------------- the plan
def clp_plan(shapes: Sequence[Sequence[int]]) -> List[tuple]:
    """Step 1: ``[(kind, index), ...]`` from the layers' shapes."""
    nd = [len(s) for s in shapes]
    plan, at = [], 0
    while at < len(nd):
        if nd[at] == 4:
            plan.append(("conv", at))
            at += 1
        elif nd[at] == 1 and at + 3 < len(nd):
            if all(d == 1 for d in nd[at:at + 4]):
                plan.append(("bn", at))
                at += 4
            else:
                at += 1
        elif nd[at] == 2:
            plan.append(("fc", at))
            at += 1
        else:
            at += 1
    return plan


def _bn_of(plan: list, e: int):
    """The bn entry's index that conv entry ``e`` takes its scale from, or None."""
    return plan[e + 1][1] if e + 1 < len(plan) and plan[e + 1][0] == "bn" else None


# --------------------------------------------------------------- the features
def sigma_host(w: np.ndarray) -> float:
    w = np.asarray(w, np.float64)
    if not np.isfinite(w).all():  # (LAPACK raises on these: the feature is not finite, decide names the client)
        return float("nan")
    return float(np.linalg.svd(w, compute_uv=False)[0]) if w.size else 0.0


def scale_host(bn_w: np.ndarray, bn_var: np.ndarray) -> np.ndarray:
    return np.abs(bn_w.astype(np.float64)) / np.sqrt(np.maximum(bn_var.astype(np.float64), 0) + EPS)


def entry_host(layers: Sequence[np.ndarray], plan: list, e: int) -> np.ndarray:
    """Step 2 for plan entry ``e`` of one client."""
    kind, idx = plan[e]
    if kind == "bn":
        return scale_host(layers[idx], layers[idx + 3])
    w = layers[idx]
    if kind == "fc":
        return np.array([sigma_host(w.reshape(w.shape[0], -1))], np.float64)
    out = np.array([sigma_host(w[ch].reshape(w.shape[1], -1)) for ch in range(w.shape[0])], np.float64)
    bn = _bn_of(plan, e)
    if bn is not None:
        scale = scale_host(layers[bn], layers[bn + 3])
        n = min(len(scale), len(out))
        out[:n] = out[:n] * scale[:n]
    return out


def features_host(layers: Sequence[np.ndarray], plan: list) -> List[np.ndarray]:
    """Step 2 for one client: one float64 array per plan entry; for an empty
    plan the one array of the layers' norms."""
    with np.errstate(over="ignore", invalid="ignore"):
        if not plan:
            return [np.array([np.sqrt(np.sum(np.square(x.astype(np.float64).reshape(-1)))) for x in layers], np.float64)]
        return [entry_host(layers, plan, e) for e in range(len(plan))]


# -------------------------------------------------------------- the decisions
def decide(features: Sequence[Sequence[np.ndarray]], plan: list, threshold: float) -> dict:
    """Step 3: ``features[i]`` is client ``i``'s arrays (``features_host``),
    wherever they were computed.  Labels (0 kept, -1 left out), every client's
    kept features, their count and the distance matrix."""
    from scipy.stats import wasserstein_distance
    from sklearn.cluster import KMeans

    C = len(features)
    for i, fs in enumerate(features):
        if not all(np.isfinite(f).all() for f in fs):
            raise ValueError(f"client {i}: non-finite parameters (a NaN, an infinity or an overflowing sum): MARS's "
                             f"Lipschitz constants are undefined")
    vecs = []
    for fs in features:
        fs = [np.asarray(f, np.float64) for f in fs]
        kept = [f[f >= np.quantile(f, 1 - TOP)] for f in fs if f.size] if plan else fs
        vecs.append(np.concatenate(kept) if kept else np.zeros(0))
    hist = [np.histogram(v, bins=50, density=True)[0] if len(v) else None for v in vecs]
    D = np.zeros((C, C), np.float64)
    for i in range(C):
        for j in range(i + 1, C):
            if hist[i] is not None and hist[j] is not None:
                D[i, j] = D[j, i] = wasserstein_distance(hist[i], hist[j])
    labels = np.zeros(C, dtype=int)
    if C >= 2:
        km = KMeans(n_clusters=2, random_state=42, n_init=10).fit(D).labels_
        centres = []
        for k in range(2):
            members = [vecs[i] for i in range(C) if km[i] == k]
            if members:
                centres.append(np.histogram(np.concatenate(members), bins=50, density=True)[0])
        if len(centres) == 2 and wasserstein_distance(centres[0], centres[1]) > threshold:
            # (two centres: both clusters have members, so a centre's position is its cluster's number)
            bad = int(np.argmax([np.linalg.norm(c, ord=1) for c in centres]))
            labels = np.where(km == bad, -1, 0)
    return {"labels": [int(v) for v in labels], "features": vecs, "kept_counts": [len(v) for v in vecs],
            "distances": D}


# ------------------------------------------------------------------ the whole
def mars_host(data: Sequence[Sequence[np.ndarray]], weights=None, threshold: float = 1.0) -> tuple:
    """The whole definition on host arrays: ``data[i][l]`` is client ``i``'s
    layer ``l``.  Returns (the float64 layers, the report)."""
    data = [[np.asarray(x) for x in d] for d in data]
    C = len(data)
    layers = _layers(data)
    _one_type(layers)
    w = _weights(weights, C)
    plan = clp_plan([x.shape for x in data[0]])
    report = decide([features_host(d, plan) for d in data], plan, threshold)
    report["host_layers"] = len(plan) if plan else len(layers)
    kept = [i for i in range(C) if report["labels"][i] == 0]
    if not kept:
        return [x.copy() for x in data[0]], report
    return [average_host([xs[i] for i in kept], [w[i] for i in kept]) for xs in layers], report


class MarsAggregator(RobustAggregator):
    """MARS aggregator (Lipschitz-based Byzantine-robust aggregation).

    The computation is performed in plaintext.  ``average`` over the parties
    runs the module's definition; when any layer of the uploads is a CUDA
    tensor the features of the whole model are computed on that device (host
    layers among them go there through pinned memory) by ``sa_mars_sigma`` and
    ``sa_mars_bn``, read back in one pinned read, and the kept clients are
    averaged there: a list of float64 tensors on the device.  Uploads that are
    all host arrays run the numpy form and give float64 arrays.  ``sum`` is
    ``RobustAggregator.sum`` (the reference inherits ``PlainAggregator.sum``).

    After each ``average``, ``last_report`` holds ``labels`` (0 kept, -1 left
    out), ``features`` (every client's kept Lipschitz constants),
    ``kept_counts``, ``distances`` and ``host_layers`` (the plan entries whose
    features were computed on the host); the device path adds ``wide_layers``
    (the plan entries that took ``sa_mars_sigma_wide``).

    ``wide_layers`` says where a layer with a smaller side above 32 goes on
    the device path: ``"host"`` (the default) reads it to the host for LAPACK,
    ``"device"`` keeps it on the device up to a smaller side of 512.

    Examples:
      >>> aggregator = MarsAggregator(server, anomaly_threshold=1.0)
      >>> fl = FLModel(server=server, device_list=clients, model=build, aggregator=aggregator)
    """

    def __init__(self, device: PYU, anomaly_threshold: float = 1.0, wide_layers: str = "host"):
        super().__init__(device)
        if wide_layers not in ("host", "device"):
            raise ValueError(f"wide_layers is 'host' or 'device', not {wide_layers!r}")
        self.anomaly_threshold = anomaly_threshold
        self.wide_layers = wide_layers

    # ------------------------------------------------------------ the paths
    def _device_features(self, layers: list, on_dev: list, plan: list, dev) -> tuple:
        """Every client's arrays of step 2 and the numbers of plan entries that went to the host and to the
        wide kernels."""
        from ... import _lib as L
        from ... import hostpipe as H
        from ... import kernels as K

        C = len(on_dev[0])
        shapes = [tuple(xs[0].shape) for xs in layers]
        sizes = [shapes[idx][0] if kind != "fc" else 1 for kind, idx in plan]
        offsets = np.concatenate([[0], np.cumsum([C * n for n in sizes])]).astype(int)
        buf = torch.zeros(int(offsets[-1]), dtype=torch.float64, device=dev)
        dims = {e: (shapes[idx][0], shapes[idx][1], int(np.prod(shapes[idx][2:]))) if kind == "conv"
                else (1,) + shapes[idx] for e, (kind, idx) in enumerate(plan) if kind != "bn"}
        # the entries for sa_mars_sigma_wide, and one scratch for the largest of them, reused in stream order
        wide = {}
        for e, (n_mat, rows, cols) in dims.items():
            if self.wide_layers == "device" and n_mat and MAX_P < min(rows, cols) <= WIDE_MAX_P:
                need = L.lib().sa_mars_wide_scratch_bytes(C, n_mat, rows, cols)
                if need >= 0:  # (a size the library refuses: to the host like a wider one)
                    wide[e] = need
        scratch = torch.empty(max(wide.values()) // 8, dtype=torch.float64, device=dev) if wide else None
        on_host = {}
        for e, (kind, idx) in enumerate(plan):
            off = int(offsets[e])
            if kind == "bn":
                K.mars_bn(on_dev[idx], on_dev[idx + 3], buf, off)
                continue
            n_mat, rows, cols = dims[e]
            bn = _bn_of(plan, e) if kind == "conv" else None
            scale = dict(bn_w=on_dev[bn], bn_var=on_dev[bn + 3]) if bn is not None else {}
            if e in wide:
                K.mars_sigma_wide(on_dev[idx], n_mat, rows, cols, scratch, buf, off, **scale)
            elif not 1 <= min(rows, cols) <= MAX_P or n_mat == 0:
                # beyond the kernels' size: this entry's layers through pinned memory, LAPACK on the host
                need = [idx] if bn is None else [idx, bn, bn + 3]
                on_host[e] = [entry_host({l: H.d2h(on_dev[l][i], pooled=False).reshape(shapes[l]) for l in need},
                                         plan, e) for i in range(C)]
            else:
                K.mars_sigma(on_dev[idx], n_mat, rows, cols, buf, off, **scale)
        flat = H.d2h(buf, pooled=False) if buf.numel() else np.zeros(0)  # the one read of the features
        feats = [[on_host[e][i] if e in on_host else flat[offsets[e] + i * n:offsets[e] + (i + 1) * n]
                  for e, n in enumerate(sizes)] for i in range(C)]
        return feats, len(on_host), len(wide)

    def _device_average(self, layers: list, w: List[float], dev) -> list:
        from ... import hostpipe as H

        on_dev = upload(layers, dev, "MarsAggregator")
        C = len(layers[0])
        plan = clp_plan([tuple(xs[0].shape) for xs in layers])
        if plan:
            feats, host_layers, wide_layers = self._device_features(layers, on_dev, plan, dev)
        else:  # the fallback's norms: every layer on the host
            hosts = [[H.d2h(row[i], pooled=False) for row in on_dev] for i in range(C)]
            feats, host_layers, wide_layers = [features_host(h, plan) for h in hosts], len(layers), 0
        report = decide(feats, plan, self.anomaly_threshold)
        report["host_layers"], report["wide_layers"] = host_layers, wide_layers
        self.last_report = report
        keep = [lb == 0 for lb in report["labels"]]
        if not any(keep):
            return [row[0].clone().reshape(tuple(xs[0].shape)) for xs, row in zip(layers, on_dev)]
        return average_kept(layers, on_dev, w, keep, dev)

    def _average(self, parties: list, weights):
        single, data, layers, w, dev = self._parse(parties, weights, one_type=True)
        if dev is not None:
            outs = self._device_average(layers, w, dev)
        else:
            outs, self.last_report = mars_host([[_host(x) for x in d] for d in data], w, self.anomaly_threshold)
        log.info("Anomaly detection results: %s", self.last_report["labels"])
        return outs[0] if single else outs
