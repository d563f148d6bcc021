"""QuantizedKmeans restated in plain Python integers, looped over elements and
clusters: the definition of sfl_amd/utils/quantized.py's docstring and
DESIGN.md section 18, sharing no code with the package (tests/test_kmeans_oracle.py
checks it on hand-worked cases first).  Floats are Python floats (float64);
``round`` is round-half-to-even as ``rint``.

``variant`` turns the step into one of four wrong implementations, for the
tests that show which case tells each of them from the definition:
``"float_sums"`` (the sums added in float64 in element order), ``"sum32"``
(a 32-bit sum), ``"le"`` (an element on a boundary goes up: ``b_j <= u``) and
``"half_down"`` (a mean with remainder exactly ``cnt / 2`` rounds down)."""

U = (1 << 32) - 1
BINS, SHIFT = 4096, 20


def image(xs, mn, mx):
    """The 32-bit image of the values ``xs`` (Python floats) under the range ``[mn, mx]``."""
    s = float(U) / (mx - mn)
    return [max(0, min(U, int(round((x - mn) * s)))) for x in xs]  # a start may lie outside the range


def icbrt(v):
    """The largest integer w with w^3 <= v, by bisection."""
    lo, hi = 0, 1
    while hi * hi * hi <= v:
        hi *= 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if mid * mid * mid <= v:
            lo = mid
        else:
            hi = mid
    return lo


def histogram(us):
    h = [0] * BINS
    for u in us:
        h[u >> SHIFT] += 1
    return h


def start(h, K):
    """The "cbrt" start: the (2j+1)/2K quantiles of the cube root of the density."""
    w = [icbrt(c << 30) for c in h]
    tot = sum(w)
    cs = []
    for j in range(K):
        r = ((2 * j + 1) * tot) // (2 * K)
        below, b = 0, 0
        while below + w[b] <= r:  # the first bin whose inclusive prefix sum exceeds r
            below += w[b]
            b += 1
        cs.append((b << SHIFT) + (((r - below) << SHIFT) // w[b]))
    return cs


def labels(us, c, variant=None):
    bs = [(c[j] + c[j + 1]) >> 1 for j in range(len(c) - 1)]
    if variant == "le":
        return [sum(1 for b in bs if b <= u) for u in us]
    return [sum(1 for b in bs if b < u) for u in us]


def step(us, c, variant=None):
    """One Lloyd step: the new centres."""
    K = len(c)
    cnt, tot = [0] * K, [0.0 if variant == "float_sums" else 0] * K
    for u, l in zip(us, labels(us, c, variant)):
        cnt[l] += 1
        tot[l] += u
    new = []
    for j in range(K):
        if cnt[j] == 0:
            new.append(c[j])
            continue
        t = int(tot[j]) & 0xFFFFFFFF if variant == "sum32" else int(tot[j])
        quo, rem = divmod(t, cnt[j])
        up = 2 * rem > cnt[j] if variant == "half_down" else 2 * rem >= cnt[j]
        new.append(quo + (1 if up else 0))
    return new


def fit(xs, K, init="cbrt", max_iter=50, variant=None):
    """``(labels, c, n_iter, q)`` of the values ``xs`` (a list of Python
    floats): the labels under the final centres, the centres as integers, the
    steps taken and the centres as float64 (to be rounded to the data's type)."""
    mn, mx = min(xs), max(xs)
    us = image(xs, mn, mx)
    c = start(histogram(us), K) if isinstance(init, str) else image(list(init), mn, mx)
    n_iter = 0
    while n_iter < max_iter:
        new = step(us, c, variant)
        n_iter += 1
        same = new == c
        c = new
        if same:
            break
    width = (mx - mn) / float(U)
    return labels(us, c, variant), c, n_iter, [mn + float(cj) * width for cj in c]
