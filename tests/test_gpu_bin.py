"""HomoBinning on the GPU (sa_bin_range / sa_bin_ranks): the device form
equals brute force bit for bit, in both kernel forms, and a fit with a device
party equals the all-host fit."""
import numpy as np
import pytest
from bin_cases import ABNORMAL, brute_range, brute_ranks, make_case
from gpu_copies import DEV, _dev, _host

pytestmark = pytest.mark.gpu

from sfl_amd import kernels as K  # noqa: E402
from sfl_amd.preprocessing.binning import HomoBinning  # noqa: E402
from sfl_amd.preprocessing.binning.homo_binning import DeviceWorker  # noqa: E402


def _ranks(x, q, abnormal=(), misalign=False, dirty_twice=False):
    """``bin_ranks`` of host ``x`` and ascending ``q`` on the device, as a host array."""
    import torch

    xd = _dev(x, misalign).view(x.shape)
    out = torch.empty(q.shape, dtype=torch.int64, device=DEV)
    for _ in range(2 if dirty_twice else 1):
        out.fill_(-1)  # 0xFF in every byte
        got = _host(K.bin_ranks(xd, _dev(q).view(q.shape), abnormal, out))
        assert np.array_equal(got, brute_ranks(x, q, abnormal))
    return xd


def _range(x, xd, abnormal=()):
    import torch

    out = torch.full((x.shape[1], 4), -1, dtype=torch.int64, device=DEV)
    got = _host(K.bin_range(xd, abnormal, out))
    mn, mx, count, missing = brute_range(x, abnormal)
    assert np.array_equal(got[:, 0], mn.view(np.int64)) and np.array_equal(got[:, 1], mx.view(np.int64))
    assert np.array_equal(got[:, 2], count) and np.array_equal(got[:, 3], missing)


CASES = [(rows, 5, 10, "f4") for rows in (1, 63, 64, 65, 257, 4100, 70003)] \
    + [(4100, f, q, "f4") for f in (1, 3, 33, 64, 65, 130) for q in (10, 33)] \
    + [(4100, 5, q, "f4") for q in (1, 16, 17, 33, 255)] \
    + [(70003, 5, 33, "f4"), (4100, 65, 255, "f4")] \
    + [(4100, f, q, "f8") for f, q in ((5, 10), (5, 33), (65, 16), (33, 255))]


@pytest.mark.parametrize("rows,nf,q,xt", CASES)
def test_device_equals_brute_force(rows, nf, q, xt):
    x, qs = make_case(rows, nf, q, np.dtype(xt).type)
    xd = _ranks(x, qs, ABNORMAL)
    _range(x, xd, ABNORMAL)
    assert K.bin_geometry(q, nf, xd.dtype)[0] == (q > 16)


@pytest.mark.parametrize("xt", ["f4", "f8"])
@pytest.mark.parametrize("q", [10, 33])
def test_views_offset_by_one_element(xt, q):
    x, qs = make_case(4100, 5, q, np.dtype(xt).type)
    _range(x, _ranks(x, qs, misalign=True))


@pytest.mark.parametrize("q", [8, 33])
def test_strictness_and_the_float32_rounding(q):
    """Query points on data values, one float64 step to either side of them,
    and beyond float32's range on both sides."""
    n = (q - 2) // 3
    vals = np.sort(np.random.default_rng(q).standard_normal(n).astype(np.float32)).astype(np.float64)
    qs = np.sort(np.concatenate([vals, np.nextafter(vals, -np.inf), np.nextafter(vals, np.inf),
                                 [-1e300, 3.5e38, 1e300][:q - 3 * n]]))[None, :]
    x = np.concatenate([vals.astype(np.float32), np.float32([np.inf, -np.inf, 3.4028235e38, -3.4028235e38])])[:, None]
    assert qs.shape[1] == q and (brute_ranks(x, qs)[0, 1:] != brute_ranks(x, qs)[0, :-1]).any()
    _ranks(np.repeat(x, 3, axis=0), qs)


@pytest.mark.parametrize("q", [10, 33])
@pytest.mark.parametrize("at", [0, 63, 64, 4099])
def test_one_decisive_row(at, q):
    x = np.full((4100, 3), 9.0, dtype=np.float32)
    x[at] = -9.0
    qs = np.tile(np.linspace(-1, 1, q), (3, 1))
    _range(x, _ranks(x, qs))


@pytest.mark.parametrize("q", [10, 33])
def test_all_rows_in_one_bin_over_dirty_output_twice(q):
    x = np.zeros((70003, 4), dtype=np.float32)
    _ranks(x, np.tile(np.linspace(-1, 1, q), (4, 1)), dirty_twice=True)


def test_columns_without_a_valid_value():
    x, qs = make_case(257, 3, 10)
    x[:, 0], x[:, 2] = np.nan, ABNORMAL[0]
    _range(x, _ranks(x, qs, ABNORMAL), ABNORMAL)
    w = DeviceWorker(_dev(x).view(x.shape), ABNORMAL).range()
    assert w[0][0] == np.inf and w[1][2] == -np.inf and w[2].tolist()[::2] == [0, 0] and w[3].tolist()[::2] == [257, 0]


def test_mixed_parties_fit_equals_the_all_host_fit():
    from sfl_amd.device import PYU, PYUObject
    from sfl_amd.security.aggregation import SecureAggregator

    rng = np.random.default_rng(3)
    parts = [np.stack([rng.standard_normal(n), rng.standard_normal(n) ** 3], axis=1).astype(np.float32)
             for n in (500, 4100)]
    parts[1][::97, 0] = np.nan
    want = HomoBinning(max_iter=6).fit_split_points(parts)
    mixed = [parts[0], _dev(parts[1]).view(parts[1].shape)]
    hb = HomoBinning(max_iter=6)
    got = hb.fit_split_points(mixed)
    assert hb.last_report["passes"] == 7 and hb.last_report["host_fallback"] == 0
    assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(got, want))
    pyus = [PYU("alice", 0), PYU("bob", 0)]
    secure = hb.fit_split_points([PYUObject(p, m) for p, m in zip(pyus, mixed)],
                                 aggregator=SecureAggregator(PYU("server", 0), pyus))
    assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(secure, want))
    many = HomoBinning(max_iter=1, abnormal_list=[1.0, 2.0, 3.0, 4.0, 5.0])
    many.fit_split_points(mixed)
    assert many.last_report["host_fallback"] == 1
