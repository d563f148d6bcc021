"""What tests/test_hist_host.py and tests/test_gpu_hist.py share: the
reference's definition of a node histogram written out plainly (a loop over
the split points, the mask ``x < t``, ``math.fsum`` of the float64 values), the
derived bound against it, and one seeded data set per shape."""
import math

import numpy as np


def fsum_reference(x, splits, grad, hess, node, n_nodes, valid, use_missing):
    """Per node a list over the features of ``[fsum(grad), fsum(hess), count]``
    rows, ``[]`` for a feature that is not valid; with ``use_missing`` one more
    row: the node's rows that are not in the last bucket."""
    x, g, h = x.astype(np.float64), grad.astype(np.float64), hess.astype(np.float64)
    out = []
    for s in range(n_nodes):
        in_node, per_feature = node == s, []
        for f, pts in enumerate(splits):
            if not valid[f]:
                per_feature.append([])
                continue
            masks = [in_node & (x[:, f] < t) for t in pts]
            if use_missing:
                masks.append(in_node & ~masks[-1] if masks else in_node)
            per_feature.append([[math.fsum(g[m]), math.fsum(h[m]), int(m.sum())] for m in masks])
        out.append(per_feature)
    return out


def assert_within_bound(lists, ref, k_grad, k_hess):
    """Counts equal; |G - ref| <= N 2^-(k + 1), likewise H: every row rounded once to the grid."""
    for got_node, ref_node in zip(lists, ref):
        for got, want in zip(got_node, ref_node):
            assert len(got) == len(want)
            for (g, h, n), (rg, rh, rn) in zip(got, want):
                assert n == rn
                assert abs(g - rg) <= rn * 2.0 ** -(k_grad + 1), (g, rg, rn)
                assert abs(h - rh) <= rn * 2.0 ** -(k_hess + 1), (h, rh, rn)


def make_case(rows, n_features, bmax, n_nodes, x_dtype=np.float32, g_dtype=np.float32, seed=0):
    """``(x, splits, grad, hess, node)``: feature 0 has ``bmax`` split points,
    the others fewer (one of them none when there are three or more), with a
    repeated point; ``x`` is drawn from the split points themselves, values
    between them, NaN and both infinities; slots ``-1 .. n_nodes - 1``."""
    rng = np.random.default_rng(seed + 1000 * rows + 10 * n_features + bmax)
    splits = []
    for f in range(n_features):
        nb = bmax if f == 0 else 0 if f == 2 else int(rng.integers(1, bmax + 1))
        pts = np.sort(rng.standard_normal(nb).astype(x_dtype).astype(np.float64))
        if nb >= 3:
            pts[1] = pts[2]
        splits.append(pts)
    pool = np.concatenate(splits + [rng.standard_normal(16), [np.nan, np.inf, -np.inf]]).astype(x_dtype)
    x = rng.choice(pool, size=(rows, n_features))
    grad = rng.standard_normal(rows).astype(g_dtype)
    hess = rng.random(rows).astype(g_dtype)
    node = rng.integers(-1, n_nodes, rows).astype(np.int32)
    return x, splits, grad, hess, node
