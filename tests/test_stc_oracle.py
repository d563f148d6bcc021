"""Sparse ternary compression on the CPU: the tests' numpy restatement
(tests/stc_oracle.py) against what the reference's own STCSparse gave
(tests/golden/stc_reference.npz, made by tests/golden/make_stc_golden.py),
and the product's host path (sfl_amd.utils.compressor) against the
restatement, bit for bit."""
import os

import numpy as np
import pytest
import torch

import stc_oracle as so

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stc_reference.npz")
N = (1, 2, 63, 64, 65, 257, 4099, 65537)
RATES = (0.0, 0.5, 0.9, 0.99, 1.0)
DTYPES = (np.float32, np.float64)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _input(seed, n, dt):
    return (np.random.default_rng(int(seed)).standard_normal(n) * 1e-2).astype(dt)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n", N)
def test_restatement_matches_the_reference_fixture(golden, dt, n):
    """Support and signs identical; |mu - mu_ref| <= the recorded
    |mu_ref - mu_exact| + 1 ulp(T): the triangle inequality through mu_exact
    (the restatement's mu is T(a float64 sum / count), within 1 ulp of
    mu_exact), not a chosen tolerance."""
    for rate in RATES:
        key = f"{np.dtype(dt).name}_{n}_{int(rate * 100)}"
        u = _input(golden[key + "_seed"], n, dt)
        m = so.mask_count(rate, n)
        assert so.threshold_is_unique(u, m), key
        sparse, _, mu, _ = so.stc(u, mask_num=m)
        assert np.array_equal(np.packbits(sparse != 0), golden[key + "_support"]), key
        assert np.array_equal(np.packbits(sparse < 0), golden[key + "_neg"]), key
        mu_ref, err = float(golden[key + "_mu_ref"]), float(golden[key + "_mu_err"])
        assert abs(float(mu) - mu_ref) <= err + so.ulp(mu_ref, dt), (key, float(mu), mu_ref, err)
        assert np.count_nonzero(sparse) <= n - m


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 65, 4099])
@pytest.mark.parametrize("rate", RATES)
def test_host_path_is_bit_equal_to_the_restatement(dt, n, rate):
    from sfl_amd.utils import compressor as Cz

    rng = np.random.default_rng(n + int(rate * 100))
    a, b, r, acc = ((rng.standard_normal(n) * s).astype(dt) for s in (1.0, 1.0, 1e-2, 1.0))
    m = so.mask_count(rate, n)
    for bb, rr, aa in ((b, r, None), (None, r, acc), (None, None, None), (b, None, None)):
        want = so.stc(a, bb, rr, m, acc=aa)
        acc_io = None if aa is None else aa.copy()
        sparse, res, mu = Cz.stc_step(a, bb, rr, rate, acc=acc_io)
        assert sparse.dtype == dt and res.dtype == dt and np.dtype(type(mu)) == dt
        assert np.array_equal(_bits(sparse), _bits(want[0]))
        assert np.array_equal(_bits(res), _bits(want[1]))
        assert _bits(np.array([mu]))[0] == _bits(np.array([want[2]]))[0]
        if aa is not None:
            assert np.array_equal(_bits(acc_io), _bits(want[3]))
    # the list form, shapes kept, and CPU tensors through the same path
    comp = Cz.STCSparse(rate)
    assert comp.name == "STC" and comp.sparse_rate == rate
    two = comp([a, b.reshape(1, -1)])
    assert np.array_equal(_bits(two[0]), _bits(so.stc(a, mask_num=m)[0]))
    assert two[1].shape == (1, n) and np.array_equal(_bits(two[1].reshape(-1)), _bits(so.stc(b, mask_num=m)[0]))
    ts, tr, _ = Cz.stc_step(torch.from_numpy(a), torch.from_numpy(b), None, rate)
    want = so.stc(a, b, None, m)
    assert np.array_equal(_bits(ts.numpy()), _bits(want[0])) and np.array_equal(_bits(tr.numpy()), _bits(want[1]))


def test_sparse_rate_is_checked_as_in_the_reference():
    from sfl_amd.utils import compressor as Cz

    for bad in (-0.1, 1.5):
        with pytest.raises(AssertionError):
            Cz.STCSparse(bad)


def test_integer_entries_take_the_numpy_path():
    from sfl_amd.utils import compressor as Cz

    a = np.array([5, -3, 0, 9], dtype=np.int64)
    b = np.array([1, 1, 1, 1], dtype=np.int64)
    sparse, res, mu = Cz.stc_step(a, b, None, 0.5)
    assert sparse.dtype == np.float64
    # u = [4, -4, -1, 8]: -1 is masked, then the tie |4|: index 0 before index 1
    assert np.array_equal(sparse, [0.0, -6.0, 0.0, 6.0]) and np.array_equal(res, [4.0, 2.0, -1.0, 2.0]) and mu == 6.0


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_ties_at_the_threshold_mask_the_lower_indices(dt):
    """Pinned difference from the reference (whose default argsort breaks
    ties arbitrarily): all |u| = 1 with alternating signs, exactly the
    indices >= mask_num survive."""
    from sfl_amd.utils import compressor as Cz

    n = 1001
    u = np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(dt)
    for rate in (0.25, 0.5, 0.999):
        m = so.mask_count(rate, n)
        for sparse in (so.stc(u, mask_num=m)[0], Cz.stc_step(u, None, None, rate)[0]):
            assert not sparse[:m].any()
            assert np.array_equal(sparse[m:], u[m:])


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_a_nan_sorts_last_and_propagates(dt):
    """Pinned: a NaN has the largest key, survives, and makes mu (so every
    element of sparse and res) NaN, as numpy's sum and multiply do."""
    from sfl_amd.utils import compressor as Cz

    u = (np.random.default_rng(3).standard_normal(257) * 1e-2).astype(dt)
    u[100] = np.nan
    want = so.stc(u, mask_num=128)
    assert np.isnan(want[2]) and np.isnan(want[0]).all()
    sparse, res, mu = Cz.stc_step(u, None, None, 128 / 257)
    assert np.array_equal(sparse, want[0], equal_nan=True) and np.array_equal(res, want[1], equal_nan=True)
    assert np.isnan(mu)
    # everything masked: the NaN is masked too and mu is 0
    sparse, res, mu = Cz.stc_step(u, None, None, 1.0)
    assert mu == 0 and not sparse.any() and np.array_equal(res, u, equal_nan=True)


def test_sa_stc_validates_before_touching_the_gpu():
    """n >= 2^32, an element type other than float32 / float64, mask_num > n
    and missing vectors are refused with SA_ERR_ARG and a message; n == 0 is
    a no-op.  None of it needs a GPU."""
    from sfl_amd import _lib as L

    lib = L.lib()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    for xt, n, m, a in ((L.SA_F32, 2**32, 1, p), (L.SA_I64, 16, 1, p), (9, 16, 1, p), (L.SA_F32, 16, 17, p),
                        (L.SA_F32, 16, 1, None)):
        assert lib.sa_stc(a, None, None, xt, n, m, p + 64, p + 128, None, None, p + 192, None) == L.SA_ERR_ARG
        assert lib.sa_last_error()
    assert lib.sa_stc(p, None, None, L.SA_F32, 16, 1, p, p + 128, None, None, p + 192, None) == L.SA_ERR_ARG  # aliasing
    assert lib.sa_stc_scratch_bytes(2**32, L.SA_F32) == L.SA_ERR_ARG
    assert lib.sa_stc_scratch_bytes(16, L.SA_I64) == L.SA_ERR_ARG
    assert lib.sa_stc_scratch_bytes(16, L.SA_F64) > 0
    assert lib.sa_stc(None, None, None, L.SA_F64, 0, 0, None, None, None, None, None, None) == L.SA_OK
    assert not buf.any()
