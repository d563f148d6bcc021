"""sa_mars_sigma_wide (the tiled Gram matrix, Householder reduction and Sturm
counts of sfl_amd/csrc/sa_mars.hip) against LAPACK, against sa_mars_sigma where
both apply, and MarsAggregator(wide_layers="device") against the host form.

The tolerance is tests/test_gpu_mars.py's, unchanged: ``(K p / 2 + 64 p + 8)
2^-53`` relative to LAPACK's value of the float64 matrix (``K + 1`` for float64
input).  Every array moves through hostpipe's pinned buffers
(tests/gpu_copies.py)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gpu_copies  # noqa: E402
import mars_oracle as O  # noqa: E402
from sfl_amd import _lib as L  # noqa: E402
from sfl_amd.security.aggregation import mars_aggregator as M  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TYPES = ["float32", "float64"]
# (n_mat, rows, cols): p = 1; p = 2, no Householder step; one step; W^T with K no multiple of 16; the first size
# sa_mars_sigma refuses; exactly one tile; a second tile row of one row; rows > cols across tiles; conv-shaped with
# n_mat > 1 past one panel of K; the limit
SHAPES = [(3, 1, 5), (3, 2, 3), (2, 3, 5), (2, 40, 17), (1, 33, 40), (1, 64, 70), (1, 65, 81), (1, 130, 67),
          (2, 49, 128), (1, 512, 520)]


def _tol(rows, cols, tname):
    p, K = min(rows, cols), max(rows, cols) + (tname == "float64")
    return (K * p / 2 + 64 * p + 8) * U


def _lapack(w):
    return np.array([np.linalg.svd(m.astype(np.float64), compute_uv=False)[0] for m in w])


def _sigma(ws, bn_w=(), bn_var=(), offset=3, wide=True, short=0):
    """kernels.mars_sigma_wide (or mars_sigma) over the clients' (n_mat, rows, cols) arrays: (C, n_mat) values; the
    buffer around them stays."""
    from sfl_amd import kernels as K

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n_mat, rows, cols = ws[0].shape
    out = torch.full((offset + len(ws) * n_mat + 2,), -7.0, dtype=torch.float64, device=gpu_copies.DEV)
    args = [[gpu_copies._dev(w) for w in ws], n_mat, rows, cols]
    if wide:
        args.append(torch.empty(K.mars_wide_scratch_bytes(len(ws), n_mat, rows, cols) // 8 - short,
                                dtype=torch.float64, device=gpu_copies.DEV))
    (K.mars_sigma_wide if wide else K.mars_sigma)(*args, out, offset, bn_w=[gpu_copies._dev(b) for b in bn_w],
                                                  bn_var=[gpu_copies._dev(b) for b in bn_var])
    got = gpu_copies._host(out)
    assert np.all(got[:offset] == -7.0) and np.all(got[-2:] == -7.0)
    return got[offset:-2].reshape(len(ws), n_mat)


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_sigma_against_lapack(shape, tname):
    rng = np.random.default_rng(sum(shape))
    ws = [(rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 3)).astype(tname) for _ in range(2)]
    got, again = _sigma(ws), _sigma(ws)
    want = np.stack([_lapack(w) for w in ws])
    ratio = np.abs(got - want) / want / _tol(shape[1], shape[2], tname)
    print(f"{shape} {tname}: max |sigma - lapack| / tolerance = {ratio.max():.3e}")
    assert np.all(ratio <= 1)
    assert np.array_equal(got, again)  # the same bits on every run


@pytest.mark.parametrize("tname", TYPES)
def test_sigma_of_special_matrices(tname):
    rng = np.random.default_rng(5)
    w = rng.standard_normal((6, 40, 44)).astype(tname)
    w[0] = 0  # all zero: exactly +0.0
    w[1][:, 3] = w[1][:, 1]  # rank deficient
    w[2][:] = 0
    w[2][0, 0], w[2][1, 1] = 3, 3  # a repeated top eigenvalue; G is diagonal in its leading block: steps are skipped
    w[2][2:, 2:] = rng.standard_normal((38, 42)) * 0.01
    w[4][7, 2] = np.nan
    got = _sigma([w])[0]
    assert got[0] == 0.0 and not np.signbit(got[0])
    assert not np.isfinite(got[4]) and np.all(np.isfinite(np.delete(got, 4)))
    for m in (1, 2, 3, 5):
        want = _lapack(w[m:m + 1])[0]
        assert abs(got[m] - want) <= _tol(40, 44, tname) * want, m


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("shape", [(4, 9, 20), (2, 32, 64)])
def test_the_two_kernels_agree_where_both_apply(shape, tname):
    ws = [np.random.default_rng(3).standard_normal(shape).astype(tname)]
    wide, small = _sigma(ws), _sigma(ws, wide=False)
    assert np.all(np.abs(wide - small) <= 2 * _tol(shape[1], shape[2], tname) * small)


@pytest.mark.parametrize("tname", TYPES)
def test_bn_scale(tname):
    rng = np.random.default_rng(9)
    ws = [rng.standard_normal((5, 40, 36)).astype(tname) for _ in range(2)]
    bw = [rng.standard_normal(3).astype(tname) for _ in range(2)]  # n_bn = 3 < n_mat: matrices 3 and 4 unscaled
    bv = [rng.uniform(0.1, 2, 3).astype(tname) for _ in range(2)]
    got = _sigma(ws, bw, bv)
    for c in range(2):
        want = _lapack(ws[c])
        want[:3] *= np.abs(bw[c].astype(np.float64)) / np.sqrt(bv[c].astype(np.float64) + 1e-5)
        assert np.all(np.abs(got[c] - want) <= (_tol(40, 36, tname) + 4 * U) * want)


def test_refusals():
    with pytest.raises(L.SALibraryError, match=f"code {L.SA_ERR_UNSUPPORTED}: .*SA_MARS_WIDE_MAX_P"):
        _sigma([np.ones((1, 513, 600), np.float32)])
    with pytest.raises(ValueError, match="scratch smaller"):
        _sigma([np.ones((1, 40, 48), np.float32)], short=1)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_aggregator_keeps_a_wide_layer_on_the_device(T):
    from sfl_amd.device import PYU, PYUObject
    from sfl_amd.security.aggregation import MarsAggregator

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    data = O.planted(T, extra=[(40, 48)])  # p = 40 > SA_MARS_MAX_P
    weights = [1, 2, 3, 4, 5, 6]
    server = PYU("server", 0)
    uploads = [PYUObject(server, [gpu_copies._dev(a).reshape(a.shape) for a in d]) for d in data]
    agg = MarsAggregator(server, wide_layers="device")
    out = agg.average(uploads, axis=0, weights=weights).data
    want, host = M.mars_host(data, weights, 1.0)
    rep = agg.last_report
    assert rep["labels"] == host["labels"] == O.LABELS
    assert (rep["host_layers"], rep["wide_layers"]) == (0, 1)
    assert rep["kept_counts"] == host["kept_counts"]
    tol = _tol(40, 48, T.__name__) + 4 * U  # the largest of the model's layers' tolerances, and the scale
    for got, ref in zip(rep["features"], host["features"]):
        assert np.all(np.abs(got - ref) <= tol * ref)
    for o, w in zip(out, want):
        assert o.is_cuda and o.dtype == torch.float64 and o.shape == w.shape
        assert np.array_equal(gpu_copies._host(o), w)  # bit for bit


def test_another_value_of_the_option_is_refused():
    from sfl_amd.device import PYU
    from sfl_amd.security.aggregation import MarsAggregator

    with pytest.raises(ValueError, match="wide_layers"):
        MarsAggregator(PYU("server", 0), wide_layers="gpu")
