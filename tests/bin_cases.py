"""What tests/test_bin_host.py and tests/test_gpu_bin.py share: HomoBinning's
local quantities by brute force in float64, and one seeded data set per shape."""
import numpy as np

ABNORMAL = [-7.5]


def brute_valid(x, abnormal):
    ok = ~np.isnan(x)
    for a in abnormal:
        ok &= x != x.dtype.type(a)
    return ok


def brute_ranks(x, q, abnormal=()):
    """``#{valid x[:, f] < q[f, j]}`` per query, one mask a query."""
    valid, wide = brute_valid(x, abnormal), x.astype(np.float64)
    return np.array([[int(((wide[:, f] < t) & valid[:, f]).sum()) for t in q[f]] for f in range(x.shape[1])],
                    dtype=np.int64).reshape(q.shape)


def brute_range(x, abnormal=()):
    """``(min, max, count, missing)`` per feature: nanmin / nanmax of the valid values."""
    valid = brute_valid(x, abnormal)
    wide = np.where(valid, x.astype(np.float64), np.nan)
    some = valid.any(axis=0)
    mn = np.where(some, np.nanmin(np.where(some, wide, 0.0), axis=0), np.inf) + 0.0
    mx = np.where(some, np.nanmax(np.where(some, wide, 0.0), axis=0), -np.inf) + 0.0
    return mn, mx, valid.sum(axis=0).astype(np.int64), np.isnan(x).sum(axis=0).astype(np.int64)


def make_case(rows, n_features, n_queries, dtype=np.float32, seed=0):
    """``(x, q)``: per feature ``n_queries`` ascending float64 query points, a
    third of them values of the data's dtype, a third ``nextafter`` neighbours
    of such values in float64 on either side, the rest not representable in
    float32; ``x`` is drawn from the dtype's values nearest the query points,
    their ``nextafter`` neighbours on both sides, NaN, both infinities, both
    zeros and the abnormal value."""
    rng = np.random.default_rng(seed + 1000 * rows + 10 * n_features + n_queries)
    base = rng.standard_normal((n_features, n_queries)).astype(dtype).astype(np.float64)
    kind = rng.integers(0, 3, base.shape)
    q = np.where(kind == 1, np.nextafter(base, np.where(rng.random(base.shape) < 0.5, -np.inf, np.inf)), base)
    q = np.sort(np.where(kind == 2, base * (1 + 2.0 ** -40), q), axis=1)
    near = q.astype(dtype)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, ABNORMAL[0]], dtype=dtype)
    x = np.empty((rows, n_features), dtype=dtype)
    for f in range(n_features):
        pool = np.concatenate([near[f], np.nextafter(near[f], dtype(-np.inf)), np.nextafter(near[f], dtype(np.inf)),
                               special])
        x[:, f] = rng.choice(pool, size=rows)
    return x, q
