"""MarsAggregator's definition on the host (no GPU): the plan, the labels and
kept features against the literal restatement of the reference
(tests/mars_oracle.py), the combine against ``np.average``, the refusals."""
import numpy as np
import pytest

import mars_oracle as O
from sfl_amd.device import PYU, PYUObject
from sfl_amd.security.aggregation import MarsAggregator
from sfl_amd.security.aggregation import mars_aggregator as M

SERVER = PYU("server", None)
CONV, BN, FC = (8, 3, 3, 3), [(8,)] * 4, (10, 64)


@pytest.mark.parametrize("shapes,plan", [
    ([CONV] + BN, [("conv", 0), ("bn", 1)]),
    # a conv bias starts the group of four: the documented misparse (the BatchNorm's variance, index 5, is skipped)
    ([CONV, (8,)] + BN + [FC], [("conv", 0), ("bn", 1), ("fc", 6)]),
    ([FC, (10,), (4, 10)], [("fc", 0), ("fc", 2)]),
    ([CONV, (8,), (8,), (8,)], [("conv", 0)]),
])
def test_clp_plan(shapes, plan):
    assert M.clp_plan(shapes) == plan
    rng = np.random.default_rng(0)
    params, other = ([rng.standard_normal(s).astype(np.float32) for s in shapes] for _ in range(2))
    got = M.decide([M.features_host(p, plan) for p in (params, other)], plan, 1.0)["features"][0]
    assert np.allclose(got, O.clp(params), rtol=1e-5, atol=0)


@pytest.mark.parametrize("threshold", [1.0, 0.1, 0.01])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_planted_model_against_the_oracle(T, threshold):
    data = O.planted(T)
    weights = [1, 2, 3, 4, 5, 6]
    out = MarsAggregator(SERVER, threshold).average([PYUObject(SERVER, d) for d in data], axis=0, weights=weights).data
    _, rep = M.mars_host(data, weights, threshold)
    vectors = [O.clp(d) for d in data]
    assert rep["labels"] == O.labels(vectors, threshold) == O.LABELS
    for got, want in zip(rep["features"], vectors):
        assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-5 if T == np.float32 else 1e-12, atol=0)
    kept = [i for i, lb in enumerate(O.LABELS) if lb == 0]
    for l, o in enumerate(out):
        want = np.average([data[i][l] for i in kept], axis=0, weights=[weights[i] for i in kept])
        assert o.dtype == np.float64 and np.array_equal(o, want)


def test_refusals():
    agg, data = MarsAggregator(SERVER), O.planted(np.float32)

    def run(d, **kw):
        return agg.average([PYUObject(SERVER, x) for x in d], **kw)

    mixed = [list(d) for d in data]
    mixed[2][5] = mixed[2][5].astype(np.float64)
    with pytest.raises(ValueError, match="layer 5, client 2"):
        run(mixed)
    one_type = [[d[0], d[1].astype(np.float64)] for d in data]
    with pytest.raises(ValueError, match="layer 1"):
        run(one_type)
    shape = [list(d) for d in data]
    shape[3][10] = shape[3][10][:, :32]
    with pytest.raises(ValueError, match="layer 10, client 3"):
        run(shape)
    nan = [list(d) for d in data]
    nan[4][0] = np.full_like(nan[4][0], np.nan)
    with pytest.raises(ValueError, match="client 4: non-finite"):
        run(nan)
    with pytest.raises(ValueError, match="axis 1"):
        run(data, axis=1)
    with pytest.raises(ValueError, match="one scalar per client"):
        run(data, weights=[1.0] * 5)
