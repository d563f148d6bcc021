"""``flame_aggregator.inliers`` against sklearn's HDBSCAN with the reference's arguments at the client counts of the
wide device path (tests/test_flame_host.py covers 3 to 16 clients)."""
import numpy as np
import pytest

import flame_oracle as O
from test_flame_host import _cd  # the cosine distances of a set of points
from sfl_amd.security.aggregation import flame_aggregator as F


@pytest.mark.parametrize("C", [17, 32, 33, 64])
def test_inliers_equal_sklearn_hdbscan_at_wide_client_counts(C):
    pytest.importorskip("sklearn")
    for k in range(6):  # random directions, and a tight majority with planted outliers
        rng = np.random.default_rng(1000 * C + k)
        if k % 2 == 0:
            pts = rng.standard_normal((C, 6))
        else:
            pts = rng.standard_normal(6) + 0.05 * rng.standard_normal((C, 6))
            for i in rng.choice(C, rng.integers(1, (C - 1) // 2), replace=False):
                pts[i] = rng.standard_normal(6) * 3
        cd = _cd(pts)
        want = O.hdbscan_labels(cd)
        assert F.inliers(cd) == want, (C, k, want)
