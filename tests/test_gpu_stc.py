"""sa_stc on the GPU against the numpy restatement (tests/stc_oracle.py):
support, signs, the one magnitude, mu against an exactly rounded sum, and
the element-wise arithmetic bit for bit."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import stc_oracle as so  # noqa: E402
from gpu_copies import DEV, _bits, _dev, _host  # noqa: E402

pytestmark = pytest.mark.gpu
N = (1, 2, 63, 64, 65, 255, 256, 257, 4099, 65537, 2**20 + 3)
RATES = (0.0, 0.5, 0.9, 0.99, 1.0)
DTYPES = (np.float32, np.float64)
IDS = ["f32", "f64"]
# select passes (shift, bits) of the two key widths
PASSES = {np.float32: ((20, 11), (10, 10), (0, 10)),
          np.float64: ((52, 11), (41, 11), (30, 11), (20, 10), (10, 10), (0, 10))}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def run(a, b=None, r=None, m=0, acc=None, alias=False, misalign=False, want_mu=True):
    """(sparse, res, mu, acc') as host arrays."""
    from sfl_amd import kernels as K

    ta, tb, tr, tacc = (_dev(x, misalign) for x in (a, b, r, acc))
    sparse = _dev(np.empty_like(a), misalign)
    res = tr if alias else _dev(np.empty_like(a), misalign)
    mu = torch.full((1,), 7.0, dtype=ta.dtype, device=DEV) if want_mu else None
    scratch = torch.empty(K.stc_scratch_bytes(a.size, ta.dtype), dtype=torch.uint8, device=DEV)
    K.stc(ta, tb, tr, m, sparse, res, acc=tacc, mu_out=mu, scratch=scratch)
    torch.cuda.synchronize()
    return (_host(sparse), _host(res), None if mu is None else _host(mu)[0],
            None if acc is None else _host(tacc))


def check(a, b, r, m, acc, out):
    """The issue's four properties, for inputs without NaN / inf."""
    sparse, res, mu, acc_out = out
    dt = a.dtype
    n = a.size
    u = so.form(a, b, r)
    keep = so.keep_mask(u, m)
    exact = so.mu_exact(u, m)
    err = abs(float(mu) - exact)
    bound = so.ulp(exact, dt) if dt == np.float32 else n * 2.0**-53 * exact
    print(f"n={n} m={m} {dt.name}: mu={float(mu)!r} exact={exact!r} err={err:.3e} bound={bound:.3e}")
    assert err <= bound
    nz = keep & (u != 0) if mu != 0 else np.zeros(n, dtype=bool)
    assert np.array_equal(sparse != 0, nz)
    assert np.array_equal(sparse < 0, nz & (u < 0))
    assert np.all(_bits(np.abs(sparse[nz])) == _bits(np.array([mu], dtype=dt))[0])
    assert not _bits(sparse[~nz]).any()  # a masked position is +0
    assert np.array_equal(_bits(res), _bits(np.subtract(u, sparse)))
    if acc is not None:
        assert np.array_equal(_bits(acc_out), _bits(np.add(acc, sparse)))


_inputs = {}


def _case(dt, n):
    if (dt, n) not in _inputs:
        rng = np.random.default_rng(n)
        _inputs[(dt, n)] = tuple((rng.standard_normal(n) * s).astype(dt) for s in (1.0, 1.0, 1e-2, 1.0))
    return _inputs[(dt, n)]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", N)
def test_matches_the_restatement(dt, n):
    a, b, r, acc = _case(dt, n)
    for rate in RATES:
        m = so.mask_count(rate, n)
        check(a, b, r, m, acc, run(a, b, r, m, acc))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [257, 4099])
def test_operand_forms_alias_and_alignment(dt, n):
    """The callers' forms: worker first round (a, b), worker (a, b, r),
    after a DP pre-step (a), server first round (a, acc), server (a, r, acc);
    res_out aliasing r; vectors that are only element-aligned; no mu_out."""
    a, b, r, acc = _case(dt, n)
    m = so.mask_count(0.9, n)
    for bb, rr, aa in ((b, None, None), (b, r, None), (None, None, None), (None, None, acc), (None, r, acc)):
        check(a, bb, rr, m, aa, run(a, bb, rr, m, aa))
        check(a, bb, rr, m, aa, run(a, bb, rr, m, aa, misalign=True))
    check(a, b, r, m, None, run(a, b, r, m, alias=True))
    check(a, None, r, m, acc, run(a, None, r, m, acc, alias=True))
    with_mu, without = run(a, b, r, m), run(a, b, r, m, want_mu=False)
    assert np.array_equal(_bits(with_mu[0]), _bits(without[0])) and np.array_equal(_bits(with_mu[1]), _bits(without[1]))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_mask_none_and_all(dt):
    a = _case(dt, 4099)[0]
    sparse, res, mu, _ = run(a, m=0)
    check(a, None, None, 0, None, (sparse, res, mu, None))
    assert np.count_nonzero(sparse) == a.size
    sparse, res, mu, _ = run(a, m=a.size)
    assert mu == 0 and not _bits(sparse).any() and np.array_equal(_bits(res), _bits(a))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_equal_magnitudes_survive_from_mask_num_on(dt):
    """All |u| = 1 with alternating signs at n = 65537: exactly the indices
    >= mask_num survive.  A wave ranks 256 consecutive elements, 4 per lane,
    and a block 1024: the boundary falls inside a lane, between lanes, on a
    wave edge, on a block edge, and at both ends."""
    n = 65537
    u = np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(dt)
    for m in (1, 1846, 1848, 2304, 4096, 65535, 65536):
        sparse, res, mu, _ = run(u, m=m)
        assert mu == 1
        assert not _bits(sparse[:m]).any()
        assert np.array_equal(sparse[m:], u[m:])
        assert np.array_equal(res[:m], u[:m]) and not res[m:].any()


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_mostly_zeros(dt):
    rng = np.random.default_rng(5)
    a = (rng.standard_normal(4099) * 1e-2).astype(dt)
    a[rng.random(4099) < 0.9] = 0
    a[7] = -0.0
    for rate in (0.5, 0.9, 0.95, 0.0):
        m = so.mask_count(rate, a.size)
        check(a, None, None, m, None, run(a, m=m))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_each_select_pass_decides(dt):
    """Keys that differ in one radix digit only, from bit patterns: the
    other passes see a single bin, the digit's own pass finds the threshold."""
    ut = np.uint32 if dt == np.float32 else np.uint64
    width = 31 if dt == np.float32 else 63
    rng = np.random.default_rng(11)
    for shift, nbits in PASSES[dt]:
        digits = np.arange(1, min(2**nbits, 2001), dtype=np.uint64)  # the top digit stays below the exponent of inf
        rest = (0x2AAAAAAAAAAAAAAA & ((1 << width) - 1)) & ~(((1 << nbits) - 1) << shift)
        if shift + nbits < width:
            rest &= ~(((1 << (width - shift - nbits)) - 1) << (shift + nbits))  # then take a mid-range exponent
            rest |= (0x3F8 if dt == np.float64 else 0x3F0) << (width - 11)
        keys = (digits << np.uint64(shift)) | np.uint64(rest)
        keys = rng.permutation(keys)
        sign = rng.integers(0, 2, keys.size).astype(np.uint64) << np.uint64(width)
        a = (keys | sign).astype(ut).view(dt)
        assert np.isfinite(a).all() and np.unique(so.keys(a)).size == a.size
        for m in (1, a.size // 2, a.size - 1):
            check(a, None, None, m, None, run(a, m=m))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_denormals_next_to_huge_values(dt):
    tiny = np.float32(1e-40) if dt == np.float32 else np.float64(1e-310)
    rng = np.random.default_rng(9)
    a = (rng.integers(1, 100, 4099) * tiny).astype(dt) * rng.choice([-1, 1], 4099).astype(dt)
    a[::7] = (1e30 * rng.standard_normal(a[::7].size)).astype(dt)
    a[::13] = 0
    assert np.count_nonzero(np.abs(a) < np.finfo(dt).tiny) > 1000
    for rate in (0.3, 0.5, 0.86, 0.99):
        m = so.mask_count(rate, a.size)
        check(a, None, None, m, None, run(a, m=m))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_one_nan(dt):
    a = _case(dt, 4099)[0].copy()
    a[1234] = np.nan
    m = 2000
    sparse, res, mu, _ = run(a, m=m)
    want = so.stc(a, mask_num=m)
    assert np.isnan(mu) and np.isnan(sparse).all()
    assert np.array_equal(sparse, want[0], equal_nan=True) and np.array_equal(res, want[1], equal_nan=True)
    sparse, res, mu, _ = run(a, m=a.size)  # masked with everything else
    assert mu == 0 and not _bits(sparse).any() and np.array_equal(_bits(res), _bits(a))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_two_runs_give_identical_bits(dt):
    a, b, r, acc = _case(dt, 2**20 + 3)
    m = so.mask_count(0.9, a.size)
    one, two = run(a, b, r, m, acc), run(a, b, r, m, acc)
    for x, y in zip(one, two):
        assert np.array_equal(_bits(np.asarray(x)), _bits(np.asarray(y)))


def test_compressor_takes_the_device_path():
    """sfl_amd.utils.compressor on device tensors: device results, the
    shapes kept, equal to the kernel's."""
    from sfl_amd.utils import compressor as Cz

    a, b, r, acc = (x.reshape(4099, 1) for x in _case(np.float32, 4099))
    tacc = _dev(acc).view(acc.shape)
    sparse, res, mu = Cz.stc_step(*(_dev(x).view(a.shape) for x in (a, b, r)), 0.9, acc=tacc)
    assert sparse.is_cuda and res.is_cuda and mu.is_cuda and sparse.shape == a.shape
    m = so.mask_count(0.9, a.size)
    out = (_host(sparse).reshape(-1), _host(res).reshape(-1), _host(mu)[()], _host(tacc).reshape(-1))
    check(a.reshape(-1), b.reshape(-1), r.reshape(-1), m, acc.reshape(-1), out)
    (again,) = Cz.STCSparse(0.9)([_dev(so.form(a, b, r)).view(a.shape)])
    assert torch.equal(again, sparse)


def test_refusals_launch_nothing():
    from sfl_amd import _lib as L
    from sfl_amd import kernels as K

    lib = L.lib()
    t = torch.zeros(64, dtype=torch.float32, device=DEV)
    s = torch.empty(K.stc_scratch_bytes(64, torch.float32), dtype=torch.uint8, device=DEV)
    p = t.data_ptr()
    before = t.clone()
    for xt, n, m in ((L.SA_F32, 2**32, 1), (L.SA_F64, 2**33, 1), (L.SA_I64, 64, 1), (7, 64, 1), (L.SA_F32, 64, 65)):
        assert lib.sa_stc(p, None, None, xt, n, m, p + 64, p + 128, None, None, s.data_ptr(), None) == L.SA_ERR_ARG
        assert lib.sa_last_error()
    assert lib.sa_stc_scratch_bytes(2**32, L.SA_F32) == L.SA_ERR_ARG
    assert lib.sa_stc_scratch_bytes(64, L.SA_I64) == L.SA_ERR_ARG
    assert lib.sa_stc(None, None, None, L.SA_F32, 0, 0, None, None, None, None, None, None) == L.SA_OK  # n == 0
    torch.cuda.synchronize()
    assert torch.equal(t, before)
    with pytest.raises(ValueError):
        K.stc(t.cpu(), None, None, 1, t, t, scratch=s)  # pageable: the CPU tensor is the argument under test
