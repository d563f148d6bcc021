"""Inputs of the QuantizedKmeans tests: the seeded data of the reference
fixture (tests/golden/kmeans_reference.npz, made by
tests/golden/make_kmeans_golden.py) and the decisive-element cases, shared by
test_kmeans_host.py and test_gpu_kmeans.py."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmeans_reference.npz")
U = (1 << 32) - 1
DTYPES = (np.float32, np.float64)
DATA = ("normal", "laplace", "clumps")
KS = (8, 64)
SEEDS = tuple(range(5))  # the reference's random_state per run
CLUMPS = (-3.0, -1.0, 0.0, 0.5, 2.0, 4.0, 7.0, 9.0)
CODES_CASE = ("normal", np.float32, 8)  # the case whose codes, q and decompressed array are recorded


def data(kind, dt):
    """200,000 normal (seed 11) or Laplace (seed 12) values, or eight clumps
    of 3,000 values within 0.05 of CLUMPS (seed 13), drawn in float64 and cast."""
    if kind == "normal":
        x = np.random.default_rng(11).standard_normal(200_000)
    elif kind == "laplace":
        x = np.random.default_rng(12).laplace(size=200_000)
    else:
        rng = np.random.default_rng(13)
        x = np.concatenate([m + rng.uniform(-0.05, 0.05, 3000) for m in CLUMPS])
    return x.astype(dt)


def key(kind, dt, K):
    return f"{kind}_{np.dtype(dt).name}_k{K}"


def all_cases():
    return [(kind, dt, K) for kind in DATA for dt in DTYPES for K in KS]


def sse(x, dec):
    """The sum of squared errors in float64."""
    d = np.asarray(dec, dtype=np.float64).reshape(-1) - np.asarray(x, dtype=np.float64).reshape(-1)
    return float(np.dot(d, d))


# ---------------------------------------------------------------------------
# decisive elements: float64 data whose values are integers in [0, 2^32 - 1]
# with both ends present, so s = 1 and u = x exactly
# ---------------------------------------------------------------------------
def _place(n, pos, decisive, others, filler):
    """``n`` values: ``decisive`` at ``pos`` (negative: from the end), ``others`` at the first free
    positions, ``filler`` elsewhere."""
    assert n >= len(others) + 1
    pos = pos % n
    x = np.full(n, filler, dtype=np.float64)
    x[pos] = decisive
    free = [i for i in range(n) if i != pos][:len(others)]
    x[free] = others
    return x, pos


def boundary(n=5, pos=1):
    """``<`` against ``<=``.  K = 3 with c = [100, 301, U], a fixed point:
    b_0 = 200; cluster 0 is {0, 200, fillers 100} with mean 100, cluster 1
    {201, 401} with mean 301, cluster 2 {U}.  The element 200 lies ON b_0 and
    belongs to cluster 0, 201 = b_0 + 1 to cluster 1; an implementation that
    counts ``b_j <= u`` sends 200 up.  ``n_iter`` = 1."""
    x, pos = _place(n, pos, 200.0, [0.0, 201.0, 401.0, float(U)], 100.0)
    return dict(x=x, K=3, init=np.array([100.0, 301.0, float(U)]), max_iter=50, probe=pos, label=0, n_iter=1,
                catches="le")


def half_up(n=6, pos=2):
    """Round-half-down.  K = 3 from c = [0, 1001, U], one step: cluster 0 is
    {0, 1}, sum 1 over count 2, remainder exactly cnt / 2: c'_0 = 1.  Cluster 1
    is {501, 1501, 1001, fillers 1001} with mean 1001.  Under c' the boundary
    b_0 = (1 + 1001) >> 1 = 501 keeps the element 501 in cluster 0; rounded
    down, c'_0 = 0 gives b_0 = 500 and 501 goes to cluster 1."""
    x, pos = _place(n, pos, 501.0, [0.0, 1.0, 1501.0, 1001.0, float(U)], 1001.0)
    return dict(x=x, K=3, init=np.array([0.0, 1001.0, float(U)]), max_iter=1, probe=pos, label=0, n_iter=1,
                catches="half_down")


def sum32():
    """A 32-bit sum.  K = 2 from c = [1000, 3e9], one step: cluster 1 is
    {2e9, 3e9, 3500000001, U}, whose sum 12,794,967,296 exceeds 2^33;
    c'_1 = 3198741824 and, with c'_0 = 5e8, the element 1e9 stays in cluster 0.
    A sum kept in 32 bits gives c'_1 = 1051258176 and 1e9 goes to cluster 1."""
    x = np.array([0.0, 1e9, 2e9, 3e9, 3500000001.0, float(U)])
    return dict(x=x, K=2, init=np.array([1000.0, 3e9]), max_iter=1, probe=1, label=0, n_iter=1, catches="sum32")


SUM53_HALF = (1 << 20) + 32


def sum53():
    """Float sums.  K = 2 from c = [3 * 2^29, V], V = U - 3, one step.
    Cluster 1 is SUM53_HALF values V, then as many V + 1, then V - 2 and U:
    its sum, above 2^53, leaves remainder exactly cnt / 2, so c'_1 = V + 1.
    Cluster 0 is {0, 536870916, P} with P = 2684354559 and mean 2^30 + 1; under
    c' the boundary is (2^30 + 1 + V + 1) >> 1 = P and P stays in cluster 0.
    Added in float64 in element order the sum comes out below the true one,
    c'_1 = V, the boundary is P - 1 and P goes to cluster 1."""
    V, P = U - 3, 2684354559
    x = np.concatenate([[0.0, 536870916.0, float(P)], np.full(SUM53_HALF, float(V)), np.full(SUM53_HALF, float(V + 1)),
                        [float(V - 2), float(U)]])
    return dict(x=x, K=2, init=np.array([float(3 << 29), float(V)]), max_iter=1, probe=2, label=0, n_iter=1,
                catches="float_sums")


def empty_cluster():
    """K = 3 from c = [5, 2^31, U - 5]: cluster 1 is empty and keeps 2^31; a fixed point, ``n_iter`` = 1."""
    x = np.array([0.0, 10.0, float(U - 10), float(U)])
    return dict(x=x, K=3, init=np.array([5.0, float(1 << 31), float(U - 5)]), max_iter=50, probe=0, label=0, n_iter=1,
                catches=None)


def three_steps():
    """Twelve values (0, U and ten uniform integers, seed 1), K = 2 from the quarter points: the second
    step still moves a centre, the third moves none, ``n_iter`` = 3."""
    x = np.concatenate([[0, U], np.random.default_rng(1).integers(0, U, 10)]).astype(np.float64)
    return dict(x=x, K=2, init=np.array([float(U // 4), float(3 * (U // 4))]), max_iter=50, probe=0, label=0,
                n_iter=3, catches=None)


SMALL = dict(boundary=boundary, half_up=half_up, sum32=sum32, empty_cluster=empty_cluster, three_steps=three_steps)
POSITIONED = dict(boundary=boundary, half_up=half_up)  # the decisive element can be placed anywhere
