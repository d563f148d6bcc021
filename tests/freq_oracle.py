"""What both FreqAggregator test files share: the DCT corner by extended
precision matrix products of the tests' own basis (``np.cos`` of the plain
formula in ``np.longdouble``, no code of the package), the derived tolerances,
and the planted six-client model."""
import numpy as np

from mars_oracle import SHAPES

LD = np.longdouble
U = 2.0 ** -53
# (2, 2): a one-element feature; odd sides; the planted head; one past a 16-wide tile with a k tail; one block
# tile; one past it with the diagonal through the corner; tall (hk < h); wide (wk = q + 1 < w)
MATRICES = [(2, 2), (3, 5), (10, 64), (17, 33), (64, 64), (65, 130), (40, 6), (6, 200)]


def basis(n):
    k, i = np.arange(n, dtype=LD)[:, None], np.arange(n, dtype=LD)[None, :]
    c = np.cos(LD(np.pi if LD is np.float64 else 3.14159265358979323846264338327950288) * (2 * i + 1) * k / (2 * n))
    return c * np.sqrt(np.where(k == 0, LD(1), LD(2)) / n)


def corner(M, N):
    q = (M + N) // 4
    return min(M // 2, q + 1), min(N // 2, q + 1), q


def feature(W):
    """The ``hk x wk`` feature of ``W`` in extended precision."""
    M, N = W.shape
    hk, wk, q = corner(M, N)
    V = basis(M) @ W.astype(LD) @ basis(N).T
    i, j = np.arange(hk)[:, None], np.arange(wk)[None, :]
    return np.where(i + j > q, LD(0), V[:hk, :wk])


def tol_feature(W):
    """Per element of F: every sum is against a unit-norm basis row
    (Cauchy-Schwarz), M + N terms over the two products, a few u for the basis."""
    return (sum(W.shape) + 16) * U * float(np.linalg.norm(W.astype(LD)))


def tol_gram(Wi, Wj):
    hk, wk, _ = corner(*Wi.shape)
    L = hk * wk
    return (2 * np.sqrt(L) * (sum(Wi.shape) + 16) + L) * U * float(np.linalg.norm(Wi.astype(LD))) \
        * float(np.linalg.norm(Wj.astype(LD)))


def planted(T, seed=0):
    """tests/mars_oracle.py's layer list (the head, (10, 64), is layer [-2] with a
    bias after it): six clients a small local step away from one global model, as
    in a round of training, so that the honest four are close in cosine distance;
    clients 1 and 4 add a low-frequency pattern that dominates their head.  Two
    clusters, of four and of two: the four are kept."""
    rng = np.random.default_rng(seed)
    shapes = SHAPES + [(10,)]
    i, j = np.arange(10)[:, None], np.arange(64)[None, :]
    pattern = np.cos(np.pi * (2 * i + 1) / 20) * np.cos(np.pi * (2 * j + 1) * 2 / 128)
    base = [rng.standard_normal(s) * 0.1 for s in shapes]
    data = []
    for c in range(6):
        d = [(b + rng.standard_normal(b.shape) * 0.01).astype(T) for b in base]
        if c in (1, 4):
            d[-2] = (d[-2] + T(rng.uniform(1, 2)) * pattern).astype(T)
        data.append(d)
    return data


KEPT = [0, 2, 3, 5]
