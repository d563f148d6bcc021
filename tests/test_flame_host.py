"""FlameAggregator's definition on the host (no GPU): the median against
``np.median``, the inlier rule against sklearn's HDBSCAN and hand cases, the
combine against ``np.average``, the whole class against the literal numpy
restatement (tests/flame_oracle.py), the refusals, one FLModel round."""
import logging
import warnings

import numpy as np
import pytest

import flame_oracle as O
from sfl_amd.device import PYU, PYUObject
from sfl_amd.security.aggregation import FlameAggregator
from sfl_amd.security.aggregation import flame_aggregator as F

TYPES = (np.float32, np.float64)
SERVER = PYU("server", None)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _upload(data):
    return [PYUObject(SERVER, d) for d in data]


# ------------------------------------------------------------------- the median
@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 8, 16, 17])
def test_median_equals_numpy_bit_for_bit(C, T):
    rng = np.random.default_rng(100 * C + np.dtype(T).itemsize)
    st = (rng.standard_normal((C, 261)) * rng.choice([1e-3, 1.0, 1e6], 261)).astype(T)
    st[:, 0] = np.finfo(T).max  # an even C's add overflows to inf, as numpy's
    st[:, 1] = -np.finfo(T).max
    st[:, 2] = rng.permutation(st[:, 2])
    got = F.median_host(st)
    assert got.dtype == T
    with np.errstate(over="ignore"):
        want = np.median(st, axis=0)
    assert want.dtype == T
    assert np.array_equal(_bits(got), _bits(want))
    assert got[0] == (np.inf if C % 2 == 0 else np.finfo(T).max)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 8, 16, 17])
def test_median_of_a_nan_column_and_of_signed_zeros(C, T):
    rng = np.random.default_rng(C)
    st = rng.standard_normal((C, 4)).astype(T)
    st[rng.integers(C), 0] = np.nan
    # -0 < +0: with C // 2 negative zeros the middle is +0 (an even C: -0 + +0 = +0), with one more it is -0
    for col, negatives in ((1, C // 2), (2, C // 2 + 1)):
        z = np.array([-0.0] * negatives + [0.0] * (C - negatives), T)
        st[:, col] = rng.permutation(z)
    got = F.median_host(st)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want = np.median(st, axis=0)
    assert np.isnan(got[0]) and np.isnan(want[0])
    assert got[1] == 0 and not np.signbit(got[1])
    assert got[2] == 0 and np.signbit(got[2])
    assert np.array_equal(_bits(got[3:]), _bits(want[3:]))


# ------------------------------------------------------------------ the inliers
def _cd(points):
    unit = points / np.sqrt((points * points).sum(axis=1))[:, None]
    cd = np.clip(1 - unit @ unit.T, 0, 2)
    cd = (cd + cd.T) / 2
    np.fill_diagonal(cd, 0.0)
    return cd


def _matrices():
    """224 seeded distance matrices, C = 3 .. 16: random directions, and a
    tight majority with planted outliers."""
    out = []
    for C in range(3, 17):
        for k in range(16):
            rng = np.random.default_rng(1000 * C + k)
            if k % 2 == 0:
                pts = rng.standard_normal((C, 6))
            else:
                centre = rng.standard_normal(6)
                pts = centre + 0.05 * rng.standard_normal((C, 6))
                for i in rng.choice(C, rng.integers(1, max(2, (C - 1) // 2)), replace=False):
                    pts[i] = rng.standard_normal(6) * 3
            out.append(_cd(pts))
    return out


def test_inliers_equal_sklearn_hdbscan_with_the_references_arguments():
    pytest.importorskip("sklearn")
    cases = _matrices()
    assert len(cases) >= 200
    for cd in cases:
        want = O.hdbscan_labels(cd)
        assert F.inliers(cd) == want, (len(cd), want)


def _full(C, value):
    cd = np.full((C, C), float(value))
    np.fill_diagonal(cd, 0.0)
    return cd


def test_inliers_by_hand():
    assert F.inliers(np.zeros((1, 1))) == [0]
    assert F.inliers(_full(2, 0.7)) == [0, 0]
    assert F.inliers(_full(5, 0.3)) == [0] * 5  # all distances equal: everyone in
    far = _full(5, 0.01)
    far[2, :] = far[:, 2] = 0.9
    far[2, 2] = 0
    assert F.inliers(far) == [0, 0, -1, 0, 0]
    # two tight groups, {0, 1, 2} and {3, 4, 5, 6}: m = 4, only the second reaches it
    two = _full(7, 1.0)
    for grp, d in (((0, 1, 2), 0.001), ((3, 4, 5, 6), 0.002)):
        for a in grp:
            for b in grp:
                if a != b:
                    two[a, b] = d
    assert F.inliers(two) == [-1, -1, -1, 0, 0, 0, 0]


def test_a_zero_norm_client_is_at_distance_one():
    rng = np.random.default_rng(5)
    base = rng.standard_normal(64).astype(np.float32)
    data = [[base + 0.01 * rng.standard_normal(64).astype(np.float32)] for _ in range(4)]
    data.insert(1, [np.zeros(64, np.float32)])
    _, rep = F.flame_host(data)
    cd = rep["cosine_distances"]
    assert np.all(cd[1, [0, 2, 3, 4]] == 1.0) and cd[1, 1] == 0.0
    assert rep["labels"][1] == -1 and rep["labels"].count(0) >= 3


# ------------------------------------------------------------------- the combine
@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("C", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("weighted", [False, True])
def test_combine_equals_np_average_plus_noise_bit_for_bit(C, T, weighted):
    rng = np.random.default_rng(17 * C + weighted)
    for shape in ((1,), (33, 7)):
        xs = [rng.standard_normal(shape).astype(T) for _ in range(C)]
        g = F.median_host(np.stack(xs))
        scales = rng.uniform(0.05, 1.0, C)  # not values of T
        scales[0] = 1.0
        w = [int(v) for v in rng.integers(1, 1000, C)] if weighted else [1.0] * C
        keep = [True] * C
        if C >= 3:
            keep[1] = False  # a dropped client
        got = F.combine_host(xs, g, scales, w, keep)
        want = O.combine(xs, g, scales, w, keep)
        assert got.dtype == np.float64 and want.dtype == np.float64
        assert np.array_equal(_bits(got), _bits(want))
        if C >= 3:  # dropped means never read
            xs[1] = np.full(shape, np.nan, T)
            assert np.array_equal(_bits(F.combine_host(xs, g, scales, w, keep)), _bits(want))


# ------------------------------------------------------------ the whole class
def _planted(T, C=5, bad=(3,), loose=(2,), long=(4,), sizes=((20, 30), (401,)), seed=0):
    """A tight majority (m = 3 of 5 clients within 1 % of one direction), one
    of them 1.5 times as long (an inlier by its direction whose update is
    clipped: its norm is above the median norm), a looser honest client (10 %:
    the majority is complete before the threshold reaches it, so it is left
    out too) and a client that uploads something else."""
    rng = np.random.default_rng(seed)
    base = [rng.standard_normal(s) for s in sizes]
    data = [[((1.5 if i in long else 1.0) * b + (0.1 if i in loose else 0.01) * rng.standard_normal(b.shape)).astype(T)
             for b in base] for i in range(C)]
    for i in bad:
        data[i] = [(-4 * rng.standard_normal(b.shape)).astype(T) for b in base]
    return data


@pytest.mark.parametrize("weighted", [False, True])
def test_the_class_against_the_literal_restatement(weighted, capsys):
    data = _planted(np.float32)  # n = 1,001
    n = sum(x.size for x in data[0])
    w = [40, 10, 30, 20, 50] if weighted else None
    planted = [0, 0, -1, -1, 0]
    want, labels, _ = O.restated(data, w, labels=planted)
    agg = FlameAggregator(SERVER)
    got = agg.average(_upload(data), axis=0, weights=w).data
    assert agg.last_report["labels"] == labels == planted
    assert agg.last_report["scales"][4] < 0.5  # a kept client is clipped: the bound below is about something
    medians = [F.median_host(np.stack([d[l] for d in data])) for l in range(2)]
    worst = 0.0
    for l, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == np.float64 and a.shape == b.shape
        spread = max(np.abs(d[l] - medians[l]).max() for d in data)
        # the restatement's float32 norms: its scales are off by at most 2 (n + 2) 2^-24, relatively
        bound = spread * 2 * (n + 2) * 2.0 ** -24 + np.spacing(np.abs(b).astype(np.float32)).astype(np.float64)
        err = np.abs(a - b)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound)
    print(f"flame vs restatement: max |diff| / bound = {worst:.3e} (n = {n}, weighted = {weighted})")


def test_last_report_and_the_log_line(caplog):
    data = _planted(np.float64)
    agg = FlameAggregator(SERVER)
    with caplog.at_level(logging.INFO, logger=F.log.name):
        out = agg.average(_upload(data), axis=0).data
    assert "Cluster labels: [0, 0, -1, -1, 0]" in caplog.text
    rep = agg.last_report
    assert set(rep) == {"labels", "norms", "threshold", "scales", "cosine_distances"}
    assert rep["threshold"] == np.median(rep["norms"]) and rep["cosine_distances"].shape == (5, 5)
    assert np.all(rep["scales"] <= 1) and rep["scales"][3] < 0.1
    host, rep2 = F.flame_host(data)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(out, host))
    # statistics from outside give the same decisions
    layers = [[d[l] for d in data] for l in range(2)]
    stats = F.stats_host(layers, [F.median_host(np.stack(xs)) for xs in layers])
    assert F.decide(stats, 5)["labels"] == rep2["labels"]
    # a single entry per party instead of a layer list
    one = agg.average(_upload([d[1] for d in data]), axis=0).data
    assert isinstance(one, np.ndarray) and one.shape == (401,)


def test_sum_is_numpys():
    data = _planted(np.float32)
    got = FlameAggregator(SERVER).sum(_upload(data), axis=0).data
    for l in range(2):
        assert np.array_equal(got[l], np.sum([d[l] for d in data], axis=0))


# ------------------------------------------------------------------ the refusals
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_input_names_the_client(bad):
    data = _planted(np.float32, bad=())
    data[2][1][7] = bad
    with pytest.raises(ValueError, match="client 2"):
        FlameAggregator(SERVER).average(_upload(data), axis=0)


def test_weights_are_one_scalar_per_client():
    data = _planted(np.float32)
    agg = FlameAggregator(SERVER)
    with pytest.raises(ValueError, match="client 0's weight"):
        agg.average(_upload(data), axis=0, weights=[np.ones(401)] * 5)
    with pytest.raises(ValueError, match="one scalar per client"):
        agg.average(_upload(data), axis=0, weights=[1.0] * 4)
    with pytest.raises(ValueError, match="one scalar per client"):
        agg.average(_upload(data), axis=0, weights=np.ones((5, 401)))
    with pytest.raises(ValueError, match="axis"):
        agg.average(_upload(data), axis=1)
    ok = agg.average(_upload(data), axis=0, weights=[PYUObject(PYU("c", None), 3)] + [np.int64(2)] * 4).data
    assert ok[0].dtype == np.float64


def test_mismatched_shapes_and_types_name_the_layer_and_the_client():
    data = _planted(np.float32)
    data[4][1] = data[4][1][:-1]
    with pytest.raises(ValueError, match="layer 1, client 4"):
        FlameAggregator(SERVER).average(_upload(data), axis=0)
    data = _planted(np.float32)
    data[2][0] = data[2][0].astype(np.float64)
    with pytest.raises(ValueError, match="layer 0, client 2"):
        FlameAggregator(SERVER).average(_upload(data), axis=0)
    data = _planted(np.float32)
    data[0][0] = data[0][0].astype(np.int32)
    with pytest.raises(ValueError, match="layer 0, client 0"):
        FlameAggregator(SERVER).average(_upload(data), axis=0)


def test_cpu_tensors_run_the_host_form_and_other_tensor_types_are_refused():
    torch = pytest.importorskip("torch")
    data = _planted(np.float64)
    agg = FlameAggregator(SERVER)
    got = agg.average(_upload([[torch.from_numpy(a) for a in d] for d in data]), axis=0).data
    want, _ = F.flame_host(data)
    assert all(isinstance(a, np.ndarray) and np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, want))
    x = torch.ones(8, dtype=torch.float64)
    for bad, who in (([x.half()] * 3, "layer 0, client 0"), ([x, x.half(), x], "layer 0, client 1"),
                     ([x, x, x.float()], "layer 0, client 2")):
        with pytest.raises(ValueError, match=who):
            agg.average(_upload([[b] for b in bad]), axis=0)


# ----------------------------------------------------------------- an FLModel round
def test_one_flmodel_round_leaves_the_planted_client_out():
    torch = pytest.importorskip("torch")
    from torch import nn, optim

    from sfl_amd.ml.fl import FLModel, TorchModel, optim_wrapper

    class Poisoned(FlameAggregator):
        """Client 3's upload is replaced by a scaled random model; every call is kept."""

        def __init__(self, device):
            super().__init__(device)
            self.calls = []

        def average(self, data, axis=None, weights=None):
            rng = np.random.default_rng(len(self.calls))
            data = list(data)
            data[3] = PYUObject(data[3].device, [(25 * rng.standard_normal(np.shape(a))).astype(np.float32)
                                                 for a in data[3].data])
            self.calls.append(([[np.array(a) for a in d.data] for d in data], weights))
            return super().average(data, axis=axis, weights=weights)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = nn.Linear(4, 16), nn.Linear(16, 3)

        def forward(self, x):
            return self.b(torch.relu(self.a(x)))

    pyus = [PYU(f"client{i}", None) for i in range(5)]
    rng = np.random.default_rng(0)
    xs = [rng.standard_normal((32, 4)).astype(np.float32) for _ in pyus]
    ys = [rng.integers(0, 3, 32).astype(np.int64) for _ in pyus]
    agg = Poisoned(PYU("server", None))
    model = TorchModel(model_fn=Net, loss_fn=nn.CrossEntropyLoss, optim_fn=optim_wrapper(optim.SGD, lr=1e-2))
    fl = FLModel(server=None, device_list=pyus, model=model, aggregator=agg, strategy="fed_avg_w", backend="torch",
                 random_seed=7, train_device="cpu")
    fl.fit({p: x for p, x in zip(pyus, xs)}, {p: y for p, y in zip(pyus, ys)}, batch_size=32, epochs=1,
           aggregate_freq=1)
    assert len(agg.calls) == 2  # the initial weights, then the round
    assert agg.last_report["labels"][3] == -1 and agg.last_report["labels"].count(0) >= 3
    uploads, weights = agg.calls[-1]
    want, rep = F.flame_host(uploads, [float(np.asarray(w.data if isinstance(w, PYUObject) else w)) for w in weights])
    assert rep["labels"] == agg.last_report["labels"]
    for p in pyus:
        got = fl.get_weights(p)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert np.array_equal(_bits(np.asarray(a)), _bits(b.astype(np.asarray(a).dtype)))
