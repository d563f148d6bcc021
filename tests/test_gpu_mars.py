"""sa_mars_sigma / sa_mars_bn against LAPACK and the float64 formula, and
MarsAggregator on the device against the host form
(sfl_amd/security/aggregation/mars_aggregator.py).

sigma's tolerance, relative to LAPACK's value of the float64 matrix:
``(K p / 2 + 64 p + 8) 2^-53`` with p = min(rows, cols), K = max(rows, cols)
(K + 1 for float64 input, whose products round): the Gram matrix's K-term
float64 sums, halved by the square root; a loose cap for a backward-stable
Jacobi solve; the square root and LAPACK's own error.  Every array moves
through hostpipe's pinned buffers (tests/gpu_copies.py)."""
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
# (n_mat, rows, cols): p = 1; rows < cols with K no multiple of 4; 3x3 channels with K below and past a 4- and a
# 64-boundary; a classifier head; the one-tile / three-tile boundary; p = SA_MARS_MAX_P
SHAPES = [(5, 7, 1), (3, 3, 49), (9, 5, 9), (4, 65, 9), (1, 10, 512), (2, 33, 16), (2, 40, 17), (1, 64, 32)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _tol(rows, cols, tname):
    p, K = min(rows, cols), max(rows, cols) + (tname == "float64")
    return (K * p / 2 + 64 * p + 8) * U


def _lapack(w):
    return np.array([np.linalg.svd(m.astype(np.float64), compute_uv=False)[0] for m in w])


def _scale(bw, bv):
    return np.abs(bw.astype(np.float64)) / np.sqrt(np.maximum(bv.astype(np.float64), 0) + 1e-5)


def _sigma(ws, bn_w=(), bn_var=(), offset=3):
    """kernels.mars_sigma over the clients' (n_mat, rows, cols) arrays: (C, n_mat) values; the buffer around them stays."""
    from sfl_amd import kernels as K

    _dev()
    n_mat, rows, cols = ws[0].shape
    out = torch.full((offset + len(ws) * n_mat + 2,), -7.0, dtype=torch.float64, device=gpu_copies.DEV)
    K.mars_sigma([gpu_copies._dev(w) for w in ws], n_mat, rows, cols, out, offset,
                 bn_w=[gpu_copies._dev(b) for b in bn_w], bn_var=[gpu_copies._dev(b) for b in bn_var])
    got = gpu_copies._host(out)
    assert np.all(got[:offset] == -7.0) and np.all(got[-2:] == -7.0)
    return got[offset:-2].reshape(len(ws), n_mat)


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_sigma_against_lapack(shape, tname):
    rng = np.random.default_rng(sum(shape))
    C = 3 if shape == (9, 5, 9) else 2  # distinct data per client: a pointer-table mix-up shows
    ws = [(rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 3)).astype(tname) for _ in range(C)]
    got, again = _sigma(ws), _sigma(ws)
    want = np.stack([_lapack(w) for w in ws])
    ratio = np.abs(got - want) / want / _tol(shape[1], shape[2], tname)
    print(f"{shape} {tname}: max |sigma - lapack| / tolerance = {ratio.max():.3e}")
    assert np.all(ratio <= 1)
    assert np.array_equal(got, again)  # the same bits on every run


@pytest.mark.parametrize("tname", TYPES)
def test_sigma_of_special_matrices(tname):
    rng = np.random.default_rng(5)
    w = rng.standard_normal((6, 12, 5)).astype(tname)
    w[0] = 0  # all zero: exactly 0.0
    w[1][:, 3] = w[1][:, 1]  # rank deficient
    w[2][:] = 0
    w[2][0, 0], w[2][1, 1] = 3, 3  # a repeated top eigenvalue
    w[2][2:, 2:] = rng.standard_normal((10, 3)) * 0.1
    w[4][7, 2] = np.nan
    got = _sigma([w])[0]
    assert got[0] == 0.0 and not np.signbit(got[0])
    assert not np.isfinite(got[4]) and np.all(np.isfinite(np.delete(got, 4)))
    for m in (1, 2, 3, 5):
        want = _lapack(w[m:m + 1])[0]
        assert abs(got[m] - want) <= _tol(12, 5, tname) * want, m


def test_p_above_the_limit_is_refused_not_computed():
    with pytest.raises(L.SALibraryError, match=f"code {L.SA_ERR_UNSUPPORTED}: .*SA_MARS_MAX_P"):
        _sigma([np.ones((1, 33, 40), np.float32)])


@pytest.mark.parametrize("tname", TYPES)
def test_bn_scale_and_bn_features(tname):
    from sfl_amd import kernels as K

    rng = np.random.default_rng(9)
    ws = [rng.standard_normal((7, 4, 9)).astype(tname) for _ in range(2)]
    bw = [rng.standard_normal(5).astype(tname) for _ in range(2)]  # n_bn = 5 < n_mat: channels 5 and 6 unscaled
    bv = [rng.uniform(0.1, 2, 5).astype(tname) for _ in range(2)]
    bv[1][2] = -0.5  # a negative variance is clamped at 0
    got = _sigma(ws, bw, bv)
    for c in range(2):
        want = _lapack(ws[c])
        want[:5] *= _scale(bw[c], bv[c])
        assert np.all(np.abs(got[c] - want) <= (_tol(4, 9, tname) + 4 * U) * want)
    assert abs(got[1][2] - _lapack(ws[1])[2] * abs(float(bw[1][2])) / np.sqrt(1e-5)) <= 1e-12 * got[1][2]
    out = torch.zeros(11, dtype=torch.float64, device=_dev())
    K.mars_bn([gpu_copies._dev(b) for b in bw], [gpu_copies._dev(b) for b in bv], out, 1)
    want = np.concatenate([_scale(bw[c], bv[c]) for c in range(2)])
    assert np.all(np.abs(gpu_copies._host(out)[1:] - want) <= 4 * U * want)


# ------------------------------------------------------------------ the class
@pytest.mark.parametrize("case", ["float32", "float64", "host fc layer", "host array among device layers"])
def test_the_aggregator_on_device_tensors(case):
    from sfl_amd.device import PYU, PYUObject
    from sfl_amd.security.aggregation import MarsAggregator

    _dev()
    T = np.float64 if case == "float64" else np.float32
    data = O.planted(T, extra=[(40, 48)] if case == "host fc layer" else [])  # p = 40 > SA_MARS_MAX_P
    weights = [1, 2, 3, 4, 5, 6]
    server = PYU("server", 0)
    uploads = [PYUObject(server, [a if case.startswith("host array") and (i, l) == (2, 5) else
                                  gpu_copies._dev(a).reshape(a.shape) for l, a in enumerate(d)])
               for i, d in enumerate(data)]
    agg = MarsAggregator(server)
    out = agg.average(uploads, axis=0, weights=weights).data
    want, host = M.mars_host(data, weights, 1.0)
    rep = agg.last_report
    assert rep["labels"] == host["labels"] == O.LABELS
    assert rep["host_layers"] == (1 if case == "host fc layer" else 0)
    assert rep["kept_counts"] == host["kept_counts"]
    tol = _tol(64, 10, T.__name__) + 4 * U  # the largest of the model's layers' tolerances (K p = 640), and the scale
    for got, ref in zip(rep["features"], host["features"]):
        assert np.all(np.abs(got - ref) <= tol * ref)
    for o, w in zip(out, want):
        assert o.is_cuda and o.dtype == torch.float64 and o.shape == w.shape
        assert np.array_equal(gpu_copies._host(o), w)  # bit for bit


def test_seventeen_clients_on_the_device_are_refused():
    from sfl_amd.device import PYU, PYUObject
    from sfl_amd.security.aggregation import MarsAggregator

    dev = _dev()
    server = PYU("server", 0)
    data = [PYUObject(server, [torch.ones(8, device=dev) * i]) for i in range(17)]
    with pytest.raises(NotImplementedError, match="16"):
        MarsAggregator(server).average(data, axis=0)


def test_the_upload_takes_a_host_layer_and_refuses_a_second_device():
    """Six clients of three small layers: client 2 uploads a numpy layer among device tensors, and where a
    second device is visible client 4's layer 0 arrives from it (``average`` moves it to the server's).  The
    threshold keeps every client: the decisions are the planted case's subject, the upload is this one's."""
    from sfl_amd.device import PYU, PYUObject
    from sfl_amd.security.aggregation import MarsAggregator
    from sfl_amd.security.aggregation.robust import upload

    dev, two = _dev(), torch.cuda.device_count() >= 2
    rng = np.random.default_rng(7)
    data = [[rng.standard_normal(s).astype(np.float32) for s in ((8, 8), (8,), (4, 8))] for _ in range(6)]
    weights, server = [1, 2, 3, 4, 5, 6], PYU("server", 0)

    def place(i, l, a):
        if (i, l) == (2, 1):
            return a
        return gpu_copies._dev(a, device="cuda:1" if two and (i, l) == (4, 0) else gpu_copies.DEV).reshape(a.shape)

    uploads = [PYUObject(server, [place(i, l, a) for l, a in enumerate(d)]) for i, d in enumerate(data)]
    agg = MarsAggregator(server, anomaly_threshold=1e300)
    out = agg.average(uploads, axis=0, weights=weights).data
    want, host = M.mars_host(data, weights, 1e300)
    assert agg.last_report["labels"] == host["labels"] == [0] * 6 and agg.last_report["host_layers"] == 0
    for o, w in zip(out, want):
        assert o.device == dev and o.dtype == torch.float64 and o.shape == w.shape
        assert np.array_equal(gpu_copies._host(o), w)  # bit for bit
    if two:  # past ``average``'s move, a layer on another device is refused where it is found
        layers = [[u.data[l] for u in uploads] for l in range(3)]
        with pytest.raises(ValueError, match="layer 0, client 4: on cuda:1, the others on cuda:0"):
            upload(layers, dev, "MarsAggregator")
