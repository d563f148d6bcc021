"""HomoBinning's host form (sfl_amd/preprocessing/binning/homo_binning.py): the
local quantities against brute force, and the reference's loop on data of the
kind it was restated on.  No GPU."""
import numpy as np
import pytest
from bin_cases import ABNORMAL, brute_range, brute_ranks, make_case

from sfl_amd.ml.boost import FeatureHistogram
from sfl_amd.preprocessing.binning import HomoBinning
from sfl_amd.preprocessing.binning.homo_binning import HostWorker


def two_parties(rows=20000, seed=5):
    """A normal and a cubed-normal column, a NaN every 97th row; a tenth of the rows with the first party."""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.standard_normal(rows), rng.standard_normal(rows) ** 3], axis=1)
    x[::97, 0] = np.nan
    return [x[:rows // 10].copy(), x[rows // 10:].copy()]


class PlainSum:
    """A stub aggregator: counts its calls."""

    def __init__(self):
        self.calls = 0

    def sum(self, data, axis=None):
        self.calls += 1
        return np.sum(data, axis=axis).astype(np.float64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("abnormal", [[], ABNORMAL])
def test_host_worker_against_brute_force(dtype, abnormal):
    x, q = make_case(257, 5, 33, dtype)
    x[:, 3] = np.nan  # no valid value
    w = HostWorker(x, abnormal)
    got = w.ranks(range(5), q[:, ::-1])  # any order of the query points
    assert got.dtype == np.int64 and np.array_equal(got[:, ::-1], brute_ranks(x, q, abnormal))
    for a, b in zip(w.range(), brute_range(x, abnormal)):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert w.range()[0][3] == np.inf and w.range()[2][3] == 0 and w.range()[3][3] == 257


def test_the_loop_converges_within_the_rank_error():
    parts = two_parties()
    hb = HomoBinning(max_iter=64, allow_duplicate=True)  # the nodes' values as they are
    points = hb.fit_split_points(parts)
    rep = hb.last_report
    both = np.concatenate(parts)
    assert rep["fixed"] == 1.0 and rep["error_rank"] == 2.0
    values = np.stack(points)
    assert np.array_equal(rep["ranks"], brute_ranks(both, values))
    assert np.array_equal(rep["aim_ranks"], [np.floor(np.linspace(0, 1, 11)[1:] * (20000 - m)) for m in (207, 0)])
    off = np.abs(rep["ranks"] - rep["aim_ranks"])[rep["fixed_by_rank"]]
    assert rep["fixed_by_rank"].any() and off.max() <= rep["error_rank"]
    fh = FeatureHistogram(points)  # the result feeds the histograms unchanged
    assert fh.bind(both).max() == 10 and fh.bmax == 10


def test_max_iter_of_the_reference_stops_after_eleven_passes():
    hb = HomoBinning()
    hb.fit_split_points(two_parties())
    assert hb.last_report["passes"] == 11 and hb.last_report["fixed"] < 1.0


def test_aggregator_none_and_a_stub_give_the_same_points():
    parts = two_parties(2000)
    agg = PlainSum()
    a = HomoBinning(max_iter=3, aggregator=agg).fit_split_points(parts)
    b = HomoBinning(max_iter=3).fit_split_points([p.astype(np.float64) for p in parts])
    assert agg.calls == 1 + 4 and all(np.array_equal(u, v) for u, v in zip(a, b))
    only = HomoBinning(max_iter=3, bin_indexes=[1]).fit_split_points(parts)
    assert len(only) == 1 and np.array_equal(only[0], a[1])


def test_filtering_refusals_and_ignored_arguments():
    x = np.array([[0.0, 1.0], [1.0, 1.0], [1.0, np.nan], [1.0, -7.5]])
    hb = HomoBinning(bin_num=4, compress_thres=1, head_size=1, abnormal_list=ABNORMAL)
    points = hb.fit_split_points([x])
    assert all(np.all(np.diff(p) > hb.error) for p in points) and len(points[1]) == 1  # duplicates filtered
    assert len(HomoBinning(bin_num=4, allow_duplicate=True, abnormal_list=ABNORMAL).fit_split_points([x])[1]) == 4
    for bad in (np.inf, np.nan):
        y = x.copy()
        y[:, 1] = bad
        with pytest.raises(ValueError, match="feature 1"):
            hb.fit_split_points([x[:2], y] if bad == np.inf else [y])
    with pytest.raises(ValueError, match="bin_indexes"):
        HomoBinning(bin_indexes=[2]).fit_split_points([x])
    assert hb.last_report["host_fallback"] == 0
