"""PPBAggregator's host form (Python integers) on host arrays: the
AggregatorBase contract cases, rows that straddle a row end, and the three
refusals."""
import json
import os

import numpy as np
import pytest

from sfl_amd.device import PYU, PYUObject
from sfl_amd.security.aggregation import PPBAggregator

HERE = os.path.dirname(os.path.abspath(__file__))
CONTRACT = json.load(open(os.path.join(HERE, "golden", "aggregator_contract.json")))
PRIMES = json.load(open(os.path.join(HERE, "golden", "ppb_keys.json")))
SERVER = PYU("server", None)


def _agg(K, parties=2):
    return PPBAggregator.from_primes(SERVER, [SERVER] * parties, int(PRIMES[str(K)]["p"], 16),
                                     int(PRIMES[str(K)]["q"], 16))


def _arrays(v):
    return [np.array(x) for x in v] if np.ndim(v) == 3 else np.array(v)


@pytest.mark.parametrize("case", [k for k in CONTRACT if k != "source"])
def test_contract_cases(case):
    c = CONTRACT[case]
    a, b = _arrays(c["a"]), _arrays(c["b"])
    agg = _agg(2048)
    kw = {"weights": [np.array(w) if np.ndim(w) else w for w in c["weights"]]} if "weights" in c else {}
    call = agg.sum if case.startswith("sum") else agg.average
    got = call([PYUObject(SERVER, a), PYUObject(SERVER, b)], axis=0, **kw).data
    want = c.get("expect")
    if want is None:  # per-element weights: np.average is the contract's expectation
        want = np.average([a, b], axis=0, weights=kw["weights"])
    for g, w in zip(got, want) if isinstance(got, list) else [(got, want)]:
        assert g.dtype == np.float64
        np.testing.assert_almost_equal(g, np.array(w, np.float64), decimal=c["decimal"])


@pytest.mark.parametrize("K,count", [(128, 1), (128, 2), (128, 3), (192, 7), (2048, 36), (2048, 38), (2048, 75)])
def test_rows_that_straddle_a_row_end_round_trip(K, count):
    rng = np.random.default_rng(count)
    xs = [rng.uniform(-19, 19, count) for _ in range(3)]
    got = _agg(K, 3).sum([PYUObject(SERVER, x) for x in xs], axis=0).data
    assert got.shape == (count,) and np.abs(got - np.sum(xs, axis=0)).max() <= 3 * 2 / 10e12


@pytest.mark.parametrize("value", [-20.5, float("nan"), 2.0 ** 55 / 10e12 / 2 - 20 + 1])
def test_refusals_raise(value):
    with pytest.raises(OverflowError, match="party 1"):
        _agg(128).sum([PYUObject(SERVER, np.array([1.0, 2.0])), PYUObject(SERVER, np.array([1.0, value]))], axis=0)
