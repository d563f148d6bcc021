"""sa_freq_features / sa_freq_gram against extended-precision matrix products
of the tests' own basis (tests/freq_oracle.py), and FreqAggregator on the
device against the host form (sfl_amd/security/aggregation/freq_aggregator.py).

Tolerances (freq_oracle, derived, u = 2^-53): per element of F
``(M + N + 16) u ||W||_F``; per entry of G ``(2 sqrt(L) (M + N + 16) + L) u
||W_i||_F ||W_j||_F`` with L = hk wk.  Every array moves through hostpipe's
pinned buffers (tests/gpu_copies.py)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import freq_oracle as O  # noqa: E402
import gpu_copies  # noqa: E402
from sfl_amd.security.aggregation import freq_aggregator as F  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = -7.0


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _run(ws):
    """kernels.freq_features, then freq_gram, over the clients' matrices: (C, hk, wk) features and the packed
    Gram matrix; guard words before and after both outputs stay."""
    from sfl_amd import kernels as K

    dev = _dev()
    C, (M, N) = len(ws), ws[0].shape
    hk, wk, _ = O.corner(M, N)
    L, P = hk * wk, C * (C + 1) // 2
    dtype = torch.float32 if ws[0].dtype == np.float32 else torch.float64
    scratch = torch.empty(K.freq_scratch_bytes(M, N, C, dtype), dtype=torch.uint8, device=dev)
    feats = torch.full((2 + C * L + 2,), GUARD, dtype=torch.float64, device=dev)
    gram = torch.full((2 + P + 2,), GUARD, dtype=torch.float64, device=dev)
    K.freq_features([gpu_copies._dev(w) for w in ws], M, N, scratch, feats[2:2 + C * L])
    K.freq_gram(feats[2:2 + C * L], C, L, gram[2:2 + P])
    f, g = gpu_copies._host(feats), gpu_copies._host(gram)
    for got in (f, g):
        assert np.all(got[:2] == GUARD) and np.all(got[-2:] == GUARD)
    return f[2:-2].reshape(C, hk, wk), g[2:-2]


@pytest.mark.parametrize("tname", ["float32", "float64"])
@pytest.mark.parametrize("C", [1, 3, 16])
@pytest.mark.parametrize("shape", O.MATRICES)
def test_features_and_gram_against_extended_precision(shape, C, tname):
    rng = np.random.default_rng(sum(shape) + C)
    ws = [(rng.standard_normal(shape) * 10.0 ** rng.integers(-2, 3)).astype(tname) for _ in range(C)]
    (feats, gram), (again, gram2) = _run(ws), _run(ws)
    want = [O.feature(w) for w in ws]
    rf = max(float(np.abs(feats[c] - want[c]).max()) / O.tol_feature(ws[c]) for c in range(C))
    pairs = [(i, j) for i in range(C) for j in range(i, C)]
    rg = max(abs(float(gram[s] - np.sum(want[i] * want[j]))) / O.tol_gram(ws[i], ws[j]) for s, (i, j) in enumerate(pairs))
    print(f"{shape} C={C} {tname}: max error / tolerance: F {rf:.3e}, G {rg:.3e}")
    assert rf <= 1 and rg <= 1
    for c in range(C):  # behind the diagonal: +0.0
        assert np.array_equal(feats[c] == 0, np.asarray(want[c] == 0)) and not np.signbit(feats[c][feats[c] == 0]).any()
    assert np.array_equal(feats, again) and np.array_equal(gram, gram2)  # the same bits on every run


@pytest.mark.parametrize("case", ["float32", "float64", "host array among device layers"])
def test_the_aggregator_on_device_tensors(case):
    from sfl_amd.device import PYU, PYUObject
    from sfl_amd.security.aggregation import FreqAggregator

    _dev()
    data = O.planted(np.float64 if case == "float64" else np.float32)
    weights = [1, 2, 3, 4, 5, 6]
    server = PYU("server", 0)
    uploads = [PYUObject(server, [a if case.startswith("host array") and (i, l) == (2, len(d) - 2) else
                                  gpu_copies._dev(a).reshape(a.shape) for l, a in enumerate(d)])
               for i, d in enumerate(data)]
    agg = FreqAggregator(server)
    out = agg.average(uploads, axis=0, weights=weights).data
    want, host = F.freq_host(data, weights)
    rep = agg.last_report
    assert rep["labels"] == host["labels"] and rep["kept"] == host["kept"] == O.KEPT and rep["host_fallback"] == 0
    for o, w in zip(out, want):
        assert o.is_cuda and o.dtype == torch.float64 and o.shape == w.shape
        assert np.array_equal(gpu_copies._host(o), w)  # bit for bit
    out = agg.average(uploads, axis=0).data  # no weights: no filter
    assert agg.last_report["labels"] is None and agg.last_report["kept"] == list(range(6))
    assert all(np.array_equal(gpu_copies._host(o), w) for o, w in zip(out, F.freq_host(data)[0]))


def test_a_refused_scratch_size_falls_back_to_the_host(monkeypatch):
    from sfl_amd import _lib as L
    from sfl_amd import kernels as K
    from sfl_amd.device import PYU, PYUObject
    from sfl_amd.security.aggregation import FreqAggregator

    _dev()

    data, weights, server = O.planted(np.float32), [1] * 6, PYU("server", 0)
    agg = FreqAggregator(server)
    uploads = [PYUObject(server, [gpu_copies._dev(a).reshape(a.shape) for a in d]) for d in data]
    real = K.freq_scratch_bytes  # the library's own answer for a corner above 2^31 - 1 bytes, at the test's size
    monkeypatch.setattr(K, "freq_scratch_bytes", lambda r, c, n, t: real(40000, 40000, n, t))
    out = agg.average(uploads, axis=0, weights=weights).data
    assert agg.last_report["host_fallback"] == 1 and agg.last_report["kept"] == O.KEPT
    assert all(np.array_equal(gpu_copies._host(o), w) for o, w in zip(out, F.freq_host(data, weights)[0]))


def test_the_upload_takes_a_host_layer_and_refuses_a_second_device():
    """Six clients of three small layers, four of them near one model: client 2 uploads a numpy layer [-2]
    among device tensors, and where a second device is visible client 4's layer 0 arrives from it
    (``average`` moves it to the server's)."""
    from sfl_amd.device import PYU, PYUObject
    from sfl_amd.security.aggregation import FreqAggregator
    from sfl_amd.security.aggregation.robust import upload

    dev, two = _dev(), torch.cuda.device_count() >= 2
    rng = np.random.default_rng(11)
    shapes = ((8,), (8, 8), (8,))
    base = [rng.standard_normal(s) for s in shapes]
    data = [[((b if i < 4 else rng.standard_normal(b.shape)) + 0.01 * rng.standard_normal(b.shape)).astype(np.float32)
             for b in base] for i in range(6)]
    weights, server = [1, 2, 3, 4, 5, 6], PYU("server", 0)

    def place(i, l, a):
        if (i, l) == (2, 1):
            return a
        return gpu_copies._dev(a, device="cuda:1" if two and (i, l) == (4, 0) else gpu_copies.DEV).reshape(a.shape)

    uploads = [PYUObject(server, [place(i, l, a) for l, a in enumerate(d)]) for i, d in enumerate(data)]
    agg = FreqAggregator(server)
    out = agg.average(uploads, axis=0, weights=weights).data
    want, host = F.freq_host(data, weights)
    assert agg.last_report["labels"] == host["labels"] and agg.last_report["kept"] == host["kept"] == [0, 1, 2, 3]
    for o, w in zip(out, want):
        assert o.device == dev and o.dtype == torch.float64 and o.shape == w.shape
        assert np.array_equal(gpu_copies._host(o), w)  # bit for bit
    if two:  # past ``average``'s move, a layer on another device is refused where it is found
        layers = [[u.data[l] for u in uploads] for l in range(3)]
        with pytest.raises(ValueError, match="layer 0, client 4: on cuda:1, the others on cuda:0"):
            upload(layers, dev, "FreqAggregator")
