"""FreqAggregator's definition on the host (no GPU): the features against
extended-precision products and the reference's own dct-and-loop, the
clustering against sklearn's HDBSCAN and hand cases, the whole on a planted
model against ``np.average``."""
import numpy as np
import pytest

import freq_oracle as O
from sfl_amd.device import PYU, PYUObject
from sfl_amd.security.aggregation import FreqAggregator
from sfl_amd.security.aggregation import freq_aggregator as F

SERVER = PYU("server", None)


@pytest.mark.parametrize("shape", O.MATRICES)
def test_features_against_extended_precision(shape):
    W = np.random.default_rng(sum(shape)).standard_normal(shape)
    got, want = F.features_host(W), O.feature(W)
    assert got.shape == want.shape and got.dtype == np.float64
    ratio = float(np.abs(got - want).max()) / O.tol_feature(W)
    print(f"{shape}: max |F - reference| / tolerance = {ratio:.3e}")
    assert ratio <= 1
    assert np.array_equal(got == 0, np.asarray(want == 0)) and not np.signbit(got[got == 0]).any()


@pytest.mark.parametrize("shape", O.MATRICES)
def test_features_against_the_reference_loop(shape):
    dct = pytest.importorskip("scipy.fftpack").dct
    W = np.random.default_rng(sum(shape)).standard_normal(shape)
    rows = np.array([dct(r, type=2, norm="ortho") for r in W])  # tensorDCT, agg_freqfed.py:33-39
    V = np.array([dct(c, type=2, norm="ortho") for c in rows.T]).T
    h, w, q = shape[0] // 2, shape[1] // 2, (shape[0] + shape[1]) // 4
    want = [V[i][j] for i in range(h) for j in range(w) if i + j <= q]  # filtering, :54-58
    got = F.features_host(W)
    kept = [got[i][j] for i in range(got.shape[0]) for j in range(got.shape[1]) if i + j <= q]
    assert len(kept) == len(want) and np.abs(np.array(kept) - want).max() <= 1e-12 * np.linalg.norm(W)


@pytest.mark.parametrize("seed", range(40))
def test_clusters_against_sklearn(seed):
    HDBSCAN = pytest.importorskip("sklearn.cluster").HDBSCAN
    rng = np.random.default_rng(seed)
    for C in range(2, 17):  # 15 matrices a seed: 600 in all
        k = int(rng.integers(1, 4))
        X = rng.standard_normal((k, 5))[rng.integers(0, k, C)] + rng.standard_normal((C, 5)) * rng.choice([0.05, 0.3, 1])
        cd = F.distances(F.gram_host(list(X)), C)
        want = HDBSCAN(metric="precomputed", min_cluster_size=2, min_samples=1).fit_predict(cd.copy())
        got = F.decide(F.gram_host(list(X)), C)
        assert got["labels"] == list(want), (seed, C)  # the same partition under the same numbers
        unique, counts = np.unique(want, return_counts=True)
        assert got["kept"] == [i for i in range(C) if want[i] == unique[np.argmax(counts)]]


def _cd(points):
    """Distances of points on a line, as a matrix (no cosine involved: ``clusters`` takes any)."""
    p = np.asarray(points, np.float64)
    return np.abs(p[:, None] - p[None, :])


@pytest.mark.parametrize("points,labels,kept", [
    ([0, 0.1, 5, 5.2, 0.25], [0, 0, 1, 1, 0], [0, 1, 4]),  # two tight groups: the larger one
    ([0, 0.1, 5, 5.2], [0, 0, 1, 1], [0, 1]),  # two tight pairs: a tie, the lower number
    # the stragglers leave the root one by one: noise; three counts of two tie, -1 sorts first and wins
    ([0, 0.1, 5, 5.2, 20, 40], [0, 0, 1, 1, -1, -1], [4, 5]),
    # one pair among stragglers: no split has two clients on both sides, so no cluster is born, all are noise and kept
    ([0, 0.1, 5, 11], [-1, -1, -1, -1], [0, 1, 2, 3]),
])
def test_clusters_by_hand(points, labels, kept):
    assert F.clusters(_cd(points)) == labels and F.largest(labels) == kept


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_planted_model(T):
    data, weights = O.planted(T), [1, 2, 3, 4, 5, 6]
    agg = FreqAggregator(SERVER)
    out = agg.average([PYUObject(SERVER, d) for d in data], axis=0, weights=weights).data
    assert agg.last_report["kept"] == O.KEPT and agg.last_report["host_fallback"] == 0
    labels = agg.last_report["labels"]
    assert len({labels[i] for i in O.KEPT}) == 1 and labels[1] == labels[4] and sorted(set(labels)) == [0, 1]
    for l, o in enumerate(out):
        want = np.average([data[i][l] for i in O.KEPT], axis=0, weights=[weights[i] for i in O.KEPT])
        assert o.dtype == np.float64 and np.array_equal(o, want)
    out = agg.average([PYUObject(SERVER, d) for d in data], axis=0).data  # no weights: no filter
    assert agg.last_report["labels"] is None and agg.last_report["kept"] == list(range(6))
    assert all(np.array_equal(o, np.average([d[l] for d in data], axis=0, weights=[1.0] * 6))
               for l, o in enumerate(out))


def test_refusals():
    agg, data = FreqAggregator(SERVER), O.planted(np.float32)

    def run(d, **kw):
        return agg.average([PYUObject(SERVER, x) for x in d], weights=[1] * len(d), **kw)

    with pytest.raises(ValueError, match="client 0: .*2-D layer"):
        run([d[:-1] for d in data])  # layer [-2] is a BatchNorm vector
    with pytest.raises(ValueError, match="client 0: .*at least 2 x 2"):
        run([[d[-2][:1], d[-1]] for d in data])
    with pytest.raises(ValueError, match="one layer"):
        run([[d[-2]] for d in data])
    nan = [list(d) for d in data]
    nan[3][-2] = np.full_like(nan[3][-2], np.nan)
    with pytest.raises(ValueError, match="client 3: non-finite"):
        run(nan)
    with pytest.raises(ValueError, match="axis 1"):
        run(data, axis=1)
