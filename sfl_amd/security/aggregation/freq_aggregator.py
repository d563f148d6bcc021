"""The frequency-domain robust plaintext aggregator, mirroring the reference's
FreqFed aggregator (``examples/security/h_bd/agg_freqfed.py:26-174``): every
client's model is summarised by the low-frequency corner of the 2-D DCT of its
penultimate layer, the clients are clustered by the cosine distances of those
summaries, and only the largest cluster is averaged.

The definition (``C`` clients in list order, each a list of layers of one
float type ``T``, float32 or float64, with the same shapes in every client;
``freq_host`` below is the same text as code, and the device path computes the
features and their dot products with ``sa_freq_features`` / ``sa_freq_gram``,
include/sfl_sa.h):

1. **The matrix.**  ``W`` is a client's layer ``[-2]`` (``client_param[-2]``,
   ``:146``).  It must be 2-D, ``M x N`` with ``M >= 2`` and ``N >= 2``;
   anything else raises ``ValueError`` naming the client (the reference fails
   inside ``dct`` or produces an empty feature).
2. **The transform.**  ``V = C_M W C_N^T``, the reference's row-then-column
   DCT-II with ``norm="ortho"`` (``tensorDCT``, ``:26-41``), in float64 on
   ``W`` converted to float64.  ``C_N[k][n] = s_k cos(pi (2 n + 1) k / (2 N))``
   with ``s_0 = sqrt(1 / N)`` and ``s_k = sqrt(2 / N)`` (``basis_host``: the
   angle is reduced in integers, ``r = (2 n + 1) k mod 4 N`` folded into the
   first quadrant, so that entries of equal magnitude have equal bits and a
   quarter period is an exact zero).
3. **The filter** (``filtering``, ``:44-61``).  With ``h = M // 2``,
   ``w = N // 2`` and ``q = (M + N) // 4`` the feature is every ``V[i][j]``
   with ``i < h``, ``j < w`` and ``i + j <= q``.  Only the corner ``hk x wk``
   is ever computed, ``hk = min(h, q + 1)``, ``wk = min(w, q + 1)``; its
   entries with ``i + j > q`` are stored as ``+0.0``.  Zeros change no dot
   product, so the feature stays a dense ``hk x wk`` block.
4. **The distances** (``distances``; ``:80-87``).  From the Gram matrix
   ``G[i][j] = F_i . F_j`` in float64:
   ``cd[i][j] = 1 - G[i][j] / (max(sqrt(G[i][i]), 1e-5) * max(sqrt(G[j][j]), 1e-5))``
   and ``cd[i][i] = 0``: ``torch.nn.functional.cosine_similarity(..., eps=1e-5)``
   as the reference calls it.  A non-finite entry of ``G`` raises
   ``ValueError`` naming the client.
5. **The decision** (``clusters`` and ``decide``; ``clustering``, ``:64-114``,
   literally).  The labels are those of ``HDBSCAN(metric="precomputed",
   min_cluster_size=2, min_samples=1)``, written out without the library: with
   ``min_samples=1`` the mutual-reachability distance is the distance itself
   (``flame_aggregator``'s step 3 has the argument), so the hierarchy is the
   single-linkage tree of ``cd``; it is condensed with ``min_cluster_size=2``
   (a side of one client falls out of its cluster as noise, two sides of at
   least two clients are a true split), a cluster's stability is
   ``sum (lambda_leave - lambda_birth)`` over its clients with
   ``lambda = 1 / distance``, clusters are selected by excess of mass from the
   leaves up, and the root is never selected (no single-cluster result).
   Clusters are numbered as the library numbers them: breadth first down the
   tree, the side that Prim's walk from client 0 reaches first before the
   other.  The kept set is the members of ``unique[argmax(counts)]`` of
   ``np.unique(labels, return_counts=True)``.
6. **``weights is None``.**  The reference does no filtering at all (``:142``):
   everyone is averaged with weight 1.0 and ``last_report["labels"]`` is
   ``None``.  Weights are otherwise one finite scalar per client.
7. **Combine.**  ``np.average(kept, axis=0, weights=kept weights) + 0.0`` per
   layer over the kept clients in client order: float64 layers
   (``mars_aggregator``'s step 4; on the device ``sa_flame_combine`` with a
   zero median and unit scales).

Refinements over the reference: float64 features, where the reference has
float32 ``dct`` results whose bits depend on pocketfft's plan; float64 results
(the reference casts back to the uploads' type); the ``ValueError``s above;
the ``+ 0.0``.

Consequences worth knowing.  ``-1`` (noise) is a candidate of step 5's
``argmax`` and, sorted first by ``np.unique``, wins ties: with two pairs and
two stragglers the two stragglers are what is averaged.  A cluster is born
only where a split has at least two clients on both sides, so one tight pair
among stragglers forms no cluster at all: everyone is "noise" and everyone is
kept.  That is the reference's behaviour, reproduced and not repaired.  Fewer
than two clients have no distances: all are kept.

On the device at most 16 clients are taken; a layer whose scratch the library
refuses (above 2^31 - 1 bytes) is read to the host for its features and
counted in ``last_report["host_fallback"]``.  The host form takes any number.
"""

from __future__ import annotations

import logging
from typing import List, Sequence

import numpy as np
import torch

from .robust import RobustAggregator, _host, _layers, _one_type, _weights, average_host, average_kept, upload

EPS = 1e-5

log = logging.getLogger(__name__)


# --------------------------------------------------------------- the features
def corner(M: int, N: int) -> tuple:
    """Step 3's ``(hk, wk, q)``."""
    q = (M + N) // 4
    return min(M // 2, q + 1), min(N // 2, q + 1), q


def basis_host(rows: int, N: int) -> np.ndarray:
    """The first ``rows`` rows of step 2's ``C_N``."""
    k, n = np.arange(rows, dtype=np.int64)[:, None], np.arange(N, dtype=np.int64)[None, :]
    r = ((2 * n + 1) * k) % (4 * N)
    r = np.where(r > 2 * N, 4 * N - r, r)  # cos(2 pi - x) = cos(x)
    neg = r > N
    r = np.where(neg, 2 * N - r, r)  # cos(pi - x) = -cos(x)
    c = np.where(r == N, 0.0, np.cos(np.pi * (r / (2 * N)))) * np.sqrt(np.where(k == 0, 1.0, 2.0) / N)
    return np.where(neg, -c, c)


def _matrix(x, i: int):
    if x.ndim != 2 or min(x.shape) < 2:
        raise ValueError(f"client {i}: FreqFed's feature needs a 2-D layer [-2] of at least 2 x 2, not "
                         f"{tuple(x.shape)}")
    return x


def features_host(W: np.ndarray) -> np.ndarray:
    """Steps 2 and 3 for one client's matrix: the ``hk x wk`` float64 feature."""
    W = np.asarray(W, np.float64)
    M, N = W.shape
    hk, wk, q = corner(M, N)
    with np.errstate(over="ignore", invalid="ignore"):
        F = basis_host(hk, M) @ (W @ basis_host(wk, N).T)
    i, j = np.arange(hk)[:, None], np.arange(wk)[None, :]
    return np.where(i + j > q, 0.0, F)


def gram_host(feats: Sequence[np.ndarray]) -> np.ndarray:
    """The packed upper triangle (row by row, ``j >= i``) of step 4's ``G``."""
    flat = [np.asarray(f, np.float64).reshape(-1) for f in feats]
    with np.errstate(over="ignore", invalid="ignore"):
        return np.array([np.dot(flat[i], flat[j]) for i in range(len(flat)) for j in range(i, len(flat))], np.float64)


# -------------------------------------------------------------- the decisions
def distances(gram, C: int) -> np.ndarray:
    """Step 4 from the packed Gram matrix, wherever it was computed."""
    gram = np.asarray(gram, np.float64).reshape(-1)
    if gram.size != C * (C + 1) // 2:
        raise ValueError(f"{C * (C + 1) // 2} dot products expected for {C} clients, got {gram.size}")
    G = np.zeros((C, C), np.float64)
    G[np.triu_indices(C)] = gram
    G = np.where(np.tri(C, k=-1, dtype=bool), G.T, G)
    for ok in (np.isfinite(np.diag(G)), np.isfinite(G).all(axis=1)):  # a client's own norm first
        if not ok.all():
            raise ValueError(f"client {int(np.argmin(ok))}: non-finite parameters (a NaN, an infinity or an "
                             f"overflowing sum): FreqFed's cosine distances are undefined")
    norm = np.maximum(np.sqrt(np.diag(G)), EPS)
    cd = 1.0 - G / (norm[:, None] * norm[None, :])
    np.fill_diagonal(cd, 0.0)
    return cd


def _linkage(cd: np.ndarray) -> list:
    """The single-linkage tree as the library builds it: ``[(left, right,
    distance, size)]``, node ``C + e`` for entry ``e``, nodes below ``C`` the
    clients.  Prim's walk from client 0 (the nearest client outside the tree
    next, the first of equals); its steps sorted by distance; each joins the
    component of the step's earlier client (left) with the later one's."""
    C = len(cd)
    rest, reach, cur, steps = list(range(1, C)), [np.inf] * C, 0, []
    while rest:
        for j in rest:
            reach[j] = min(reach[j], float(cd[cur][j]))
        nxt = min(rest, key=lambda j: reach[j])
        steps.append((reach[nxt], cur, nxt))
        rest.remove(nxt)
        cur = nxt
    root, size, tree = list(range(2 * C - 1)), [1] * (2 * C - 1), []

    def find(a):
        while root[a] != a:
            a = root[a]
        return a

    for e, (d, a, b) in enumerate(sorted(steps, key=lambda s: s[0])):
        a, b = find(a), find(b)
        root[a] = root[b] = C + e
        size[C + e] = size[a] + size[b]
        tree.append((a, b, d, size[C + e]))
    return tree


def clusters(cd: np.ndarray) -> List[int]:
    """Step 5's labels: one cluster number per client, -1 for noise."""
    C = len(cd)
    if C < 2:
        return [-1] * C
    tree = _linkage(cd)
    # the condensed tree, breadth first from the root: rows (parent, child, lambda, size) in the library's
    # order, clusters numbered from C (the root) as they are born
    name, born, rows, queue, fresh = {2 * C - 2: C}, {C: 0.0}, [], [2 * C - 2], C + 1
    while queue:
        nxt = []
        for node in queue:
            left, right, d, _ = tree[node - C]
            lam = 1.0 / d if d > 0.0 else np.inf
            sizes = [tree[s - C][3] if s >= C else 1 for s in (left, right)]
            for side, n in zip((left, right), sizes):
                if min(sizes) >= 2:  # a true split: two new clusters
                    name[side], born[fresh], fresh = fresh, lam, fresh + 1
                    rows.append((name[node], name[side], lam, n))
                elif n >= 2:  # the cluster goes on under its name
                    name[side] = name[node]
                else:  # a client falls out
                    rows.append((name[node], side, lam, 1))
                if n >= 2:
                    nxt.append(side)
        queue = nxt
    # (inf - inf between identical clients is NaN, as in the library: a NaN compares false below)
    with np.errstate(invalid="ignore"):
        stability = {c: 0.0 for c in born}
        for parent, _, lam, n in rows:
            stability[parent] += (lam - born[parent]) * n
    # excess of mass, children before parents; the root is no candidate
    chosen = {c: True for c in born if c != C}
    kids = {c: [ch for p, ch, _, n in rows if p == c and n > 1] for c in born}
    for c in sorted(chosen, reverse=True):
        below = float(np.sum([stability[ch] for ch in kids[c]]))
        if below > stability[c]:
            chosen[c], stability[c] = False, below
        else:
            stack = list(kids[c])
            while stack:
                ch = stack.pop()
                chosen[ch] = False
                stack += kids[ch]
    number = {c: k for k, c in enumerate(sorted(c for c in chosen if chosen[c]))}
    up = {ch: p for p, ch, _, n in rows if n > 1}
    labels = [-1] * C
    for parent, child, _, n in rows:
        if n == 1:
            while parent not in number and parent in up:
                parent = up[parent]
            labels[child] = number.get(parent, -1)
    return labels


def largest(labels: List[int]) -> List[int]:
    """Step 5's kept set: the clients of the most frequent label, noise among the candidates."""
    unique, counts = np.unique(labels, return_counts=True)
    return [i for i, lb in enumerate(labels) if lb == unique[np.argmax(counts)]]


def decide(gram, C: int) -> dict:
    """Steps 4 and 5 from the packed Gram matrix: labels, the kept clients, the distances."""
    cd = distances(gram, C)
    labels = clusters(cd)
    return {"labels": labels, "kept": largest(labels), "distances": cd, "host_fallback": 0}


def _everyone(C: int) -> dict:
    return {"labels": None, "kept": list(range(C)), "distances": None, "host_fallback": 0}


# ------------------------------------------------------------------ the whole
def freq_host(data: Sequence[Sequence[np.ndarray]], weights=None) -> tuple:
    """The whole definition on host arrays: ``data[i][l]`` is client ``i``'s
    layer ``l``.  Returns (the float64 layers, the report)."""
    data = [[np.asarray(x) for x in d] for d in data]
    C = len(data)
    layers = _layers(data)
    _one_type(layers)
    w = _weights(weights, C)
    if weights is None:
        report = _everyone(C)
    else:
        if len(layers) < 2:
            raise ValueError("client 0: FreqFed's feature is of layer [-2]; the upload has one layer")
        report = decide(gram_host([features_host(_matrix(x, i)) for i, x in enumerate(layers[-2])]), C)
    kept = report["kept"]
    return [average_host([xs[i] for i in kept], [w[i] for i in kept]) for xs in layers], report


class FreqAggregator(RobustAggregator):
    """FreqFed aggregator (frequency-domain Byzantine-robust aggregation).

    The computation is performed in plaintext.  ``average`` over the parties
    runs the module's definition; when any layer of the uploads is a CUDA
    tensor the features of every client's layer ``[-2]`` and their dot products
    are computed on that device (host layers among them go there through
    pinned memory) by ``sa_freq_features`` and ``sa_freq_gram``, read back in
    one pinned read, and the kept clients are averaged there: a list of
    float64 tensors on the device.  Uploads that are all host arrays run the
    numpy form and give float64 arrays.  ``sum`` is ``RobustAggregator.sum``
    (the reference inherits ``PlainAggregator.sum``).

    After each ``average``, ``last_report`` holds ``labels`` (a cluster number
    per client, -1 for noise; ``None`` without weights), ``kept`` (the clients
    averaged), ``distances`` and ``host_fallback`` (1 when the features of a
    device upload were computed on the host).

    Examples:
      >>> aggregator = FreqAggregator(server)
      >>> fl = FLModel(server=server, device_list=clients, model=build, aggregator=aggregator)
    """

    def _device_gram(self, rows: list, shape: tuple, dev) -> tuple:
        """The packed Gram matrix of the clients' features and whether the host computed it."""
        from ... import _lib as L
        from ... import hostpipe as H
        from ... import kernels as K

        C, (M, N) = len(rows), shape
        try:
            need = K.freq_scratch_bytes(M, N, C, rows[0].dtype)
        except L.SALibraryError as e:
            if f"code {L.SA_ERR_UNSUPPORTED}:" not in str(e):
                raise
            return gram_host([features_host(H.d2h(x, pooled=False).reshape(M, N)) for x in rows]), 1
        hk, wk, _ = corner(M, N)
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        feats = torch.empty(C * hk * wk, dtype=torch.float64, device=dev)
        gram = torch.empty(C * (C + 1) // 2, dtype=torch.float64, device=dev)
        K.freq_features(rows, M, N, scratch, feats)
        K.freq_gram(feats, C, hk * wk, gram)
        return H.d2h(gram, pooled=False), 0  # the one read of the decisions' input

    def _device_average(self, layers: list, w: List[float], filtered: bool, dev) -> list:
        C = len(layers[0])
        on_dev = upload(layers, dev, "FreqAggregator")
        report = _everyone(C)
        if filtered:
            if len(layers) < 2:
                raise ValueError("client 0: FreqFed's feature is of layer [-2]; the upload has one layer")
            for i, x in enumerate(layers[-2]):
                _matrix(x, i)
            gram, fallback = self._device_gram(on_dev[-2], tuple(layers[-2][0].shape), dev)
            report = decide(gram, C)
            report["host_fallback"] = fallback
        self.last_report = report
        return average_kept(layers, on_dev, w, [i in report["kept"] for i in range(C)], dev)

    def _average(self, parties: list, weights):
        single, data, layers, w, dev = self._parse(parties, weights, one_type=True)
        if dev is not None:
            outs = self._device_average(layers, w, weights is not None, dev)
        else:
            outs, self.last_report = freq_host([[_host(x) for x in d] for d in data], None if weights is None else w)
        log.info("Nets for aggregation (no backdoor): %s; clusters: %s", self.last_report["kept"],
                 self.last_report["labels"])
        return outs[0] if single else outs
