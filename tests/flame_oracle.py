"""A helper, not a test: FLAME aggregation restated literally in numpy, step
by step as the reference's robust aggregator runs it (median per layer,
updates, cosine distances of the flattened raw parameters, a majority cluster,
float32 update norms, clipping to their median, ``np.average`` with weights,
a zero-variance noise term) -- written for reading, slow on purpose -- and the
exact statistics of step 2 by ``math.fsum`` over Python floats."""
import math

import numpy as np


def cosine_distances(features: np.ndarray) -> np.ndarray:
    """sklearn's ``cosine_distances`` when importable, else its formula."""
    try:
        from sklearn.metrics.pairwise import cosine_distances as cdist

        return cdist(features).astype(np.float64)
    except ImportError:
        norms = np.sqrt((features * features).sum(axis=1))
        unit = features / np.where(norms == 0, 1, norms)[:, None]
        cd = np.clip(1 - unit @ unit.T, 0, 2)
        np.fill_diagonal(cd, 0.0)
        return cd.astype(np.float64)


def hdbscan_labels(cd: np.ndarray):
    """The majority cluster by sklearn's HDBSCAN with the reference's
    arguments (the ``hdbscan`` package's API), or None without sklearn."""
    try:
        from sklearn.cluster import HDBSCAN
    except ImportError:
        return None
    n = len(cd)
    return HDBSCAN(min_cluster_size=int(n / 2 + 1), min_samples=1, allow_single_cluster=True,
                   metric="precomputed").fit(cd.copy()).labels_.tolist()


def restated(data, weights=None, labels=None):
    """The whole aggregation: ``data[i][l]`` client ``i``'s layer ``l``.
    ``labels`` are used when sklearn cannot cluster.  Returns (layers, labels,
    scales)."""
    C, L = len(data), len(data[0])
    estimated = [np.median(np.stack([np.array(data[i][l]) for i in range(C)], axis=0), axis=0) for l in range(L)]
    updates = [[np.array(data[i][l]) - estimated[l] for l in range(L)] for i in range(C)]
    features = np.stack([np.concatenate([np.array(a).flatten() for a in data[i]]) for i in range(C)], axis=0)
    found = hdbscan_labels(cosine_distances(features))
    labels = found if found is not None else list(labels)
    norms = [np.linalg.norm(np.concatenate([u.flatten() for u in updates[i]])) for i in range(C)]
    threshold = np.median(norms)
    models, kept_w, scales = [], [], []
    for i in range(C):
        scale = min(1.0, threshold / norms[i]) if norms[i] > 0 else 1.0
        scales.append(scale)
        if labels[i] == -1:
            continue
        models.append([estimated[l] + updates[i][l] * scale for l in range(L)])
        kept_w.append(weights[i] if weights is not None else 1.0)
    out = []
    for l in range(L):
        avg = np.average([m[l] for m in models], axis=0, weights=kept_w)
        out.append(avg + np.random.normal(loc=0.0, scale=0 * threshold, size=avg.shape))
    return out, labels, scales


def combine(xs, g, scales, weights, keep):
    """Steps 5 to 8 for one layer, given the scales: clip, rebuild,
    ``np.average`` over the kept clients, add the zero-variance noise."""
    T = g.dtype
    models = [g + (x - g) * T.type(s) for x, s, k in zip(xs, scales, keep) if k]
    w = [float(wt) for wt, k in zip(weights, keep) if k]
    avg = np.average(models, axis=0, weights=w)
    return avg + np.random.normal(loc=0.0, scale=0.0, size=avg.shape)


def exact_stats(layers, medians):
    """Step 2 exactly: ``layers[l][i]`` client ``i``'s layer ``l`` and the
    layers' medians.  Returns (stats, abs_sums): every statistic as the
    correctly rounded sum of its float64 summands ``t_k`` (``math.fsum``), in
    the packed order (``G``'s upper triangle row-major, then ``N``), and
    ``sum |t_k|`` beside each (numpy's pairwise sum: a scale, good to a few
    ulps), for the bound ``gamma_n sum |t_k|``."""
    C = len(layers[0])
    xs = [np.concatenate([np.asarray(layer[i], np.float64).reshape(-1) for layer in layers]) for i in range(C)]
    ds = [np.concatenate([(np.asarray(layer[i]) - g).astype(np.float64).reshape(-1)
                          for layer, g in zip(layers, medians)]) for i in range(C)]
    terms = [xs[i] * xs[j] for i in range(C) for j in range(i, C)] + [d * d for d in ds]
    return (np.array([math.fsum(t.tolist()) for t in terms]),
            np.array([float(np.abs(t).sum()) for t in terms]))
