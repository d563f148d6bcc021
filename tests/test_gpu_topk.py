"""The sa_topk kernels and sa_coo_gather on the GPU, bit for bit: against the
reference's fixture (tests/golden/topk_reference.npz), the host path of
sfl_amd/utils/sparse_compressor.py and the restatement in tests/topk_oracle.py.
Every output is a view into a larger allocation whose guard words on both
sides must come back unchanged."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import topk_cases as tc  # noqa: E402
import topk_oracle as to  # noqa: E402
from gpu_copies import DEV, _dev, _host  # noqa: E402

from sfl_amd import _lib as L  # noqa: E402
from sfl_amd import kernels as K  # noqa: E402
from sfl_amd.utils import compressor as C  # noqa: E402

pytestmark = pytest.mark.gpu
# 2^20 + 1: the first size with more than one tile per wave; 3 * 2^20 + 5: an odd tile count per wave
SMALL = (1, 255, 256, 257, 1023, 1025, 4 * 1024 + 3)
LARGE = (2**20 + 1, 3 * 2**20 + 5)
DTYPES = (np.float32, np.float64)
IDS = ["f32", "f64"]
GUARD = 64
PAT_F, PAT_I = 12345.0, -77


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def golden():
    return tc.Golden()


def _tdt(dt):
    return torch.float32 if np.dtype(dt) == np.float32 else torch.float64


def _ks(n):
    return sorted({1, n // 10, n - 1} | ({0, n} if n < 1000 else set()))


def _guarded(k, tdt, fill):
    big = torch.full((GUARD + k + GUARD,), fill, dtype=tdt, device=DEV)
    return big, big[GUARD:GUARD + k]


def _guards_intact(big, k, fill):
    g = _host(torch.cat([big[:GUARD], big[GUARD + k:]]))
    return bool(np.all(g == fill))


def _h(t):
    """A device tensor on the host; an empty one has nothing to copy."""
    if t.numel() == 0:
        return np.empty(0, dtype=np.int32 if t.dtype == torch.int32 else str(t.dtype).replace("torch.", ""))
    return _host(t).copy()


def _scratch(n, tdt):
    return torch.empty(K.topk_scratch_bytes(n, tdt), dtype=torch.uint8, device=DEV)


def _run(keys, x, k):
    """select + fill into guarded outputs: (index, data, flag) on the host."""
    n = keys.numel()
    scratch = _scratch(n, keys.dtype)
    ibig, index = _guarded(k, torch.int32, PAT_I)
    dbig, data = _guarded(k, x.dtype, PAT_F)
    flag = K.coo_flag(DEV)
    K.topk_select(keys, k, scratch)
    K.topk_fill(keys, x, k, scratch, index, data, flag)
    out = _h(index), _h(data), _h(flag)
    assert _guards_intact(ibig, k, PAT_I) and _guards_intact(dbig, k, PAT_F), "a store beyond k"
    return out


def _check(keys, x, k, want_index, x_host):
    index, data, flag = _run(keys, x, k)
    assert flag.tolist() == [0, -1]
    assert np.array_equal(index, want_index)
    assert to.same_bits(data, x_host[want_index])


# ---------------------------------------------------------------------------
# the fixture, through the classes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(tc.SHAPES)))
def test_fixture_parity_on_the_device(golden, si):
    for k, _, ri, dt in (c for c in tc.all_cases() if c[1] == si):
        x = tc.case_input(golden.seed(k), tc.SHAPES[si], tc.scale_of(ri), dt)
        comp = C.TopkSparse(tc.RATES[ri])
        host = comp.compress(x)
        xd = _dev(x).reshape(x.shape)
        c = comp.compress(xd)
        assert c.is_device and c.k == golden.k(k) and c.shape == host.shape and c.origin_shape == x.shape, k
        assert np.array_equal(_host(c.index), host.index) if c.k else c.index.numel() == 0, k
        if c.k:
            assert to.same_bits(_host(c.compressed_data), host.compressed_data), k
            assert np.array_equal(_host(c.row), host.row) and np.array_equal(_host(c.col), host.col), k
        dec = comp.decompress(c)
        assert dec.is_cuda and dec.shape == xd.shape and dec.dtype == xd.dtype, k
        assert np.array_equal(tc.digest(_host(dec.reshape(-1)).reshape(x.shape)), golden.dec(k)), k
        again = comp.decompress(comp.compress(xd, sparse_mask=c.get_sparse_mask()))  # a device mask
        assert np.array_equal(tc.digest(_host(again.reshape(-1)).reshape(x.shape)), golden.dec_mask(k)), k
        if ri == 0:  # a host mask with device data
            again = comp.decompress(comp.compress(xd, sparse_mask=host.get_sparse_mask()))
            assert np.array_equal(tc.digest(_host(again.reshape(-1)).reshape(x.shape)), golden.dec_mask(k)), k
            assert to.same_bits(c.to("cpu").to_dense(), comp.decompress(host)), k


@pytest.mark.parametrize("scheme", list(tc.MIXED))
def test_mixed_on_the_device(golden, scheme):
    cls, kw = tc.MIXED[scheme]
    for k, _, si, dt in (c for c in tc.mixed_cases() if c[1] == scheme):
        x = tc.case_input(golden.seed(k), tc.SHAPES[si], tc.SCALES[1], dt)
        comp = C.MixedCompressor(C.TopkSparse(tc.MIXED_RATE), getattr(C, cls)(**kw))
        host = comp.compress(x)
        xd = _dev(x).reshape(x.shape)
        c = comp.compress(xd)
        assert c.is_device and c.compressed_data.is_cuda, k
        codes = _host(c.compressed_data)
        assert codes.dtype == np.int8 and np.array_equal(codes, golden.codes(k)), k
        assert np.array_equal(codes, host.compressed_data), k
        dec = _host(comp.decompress(c).reshape(-1)).reshape(x.shape)
        assert np.array_equal(tc.digest(dec), golden.dec(k)), k
        assert to.same_bits(dec, comp.decompress(host)), k
    with pytest.raises(ValueError, match=r"mixed entry \[0\]: the sparse payload is empty"):
        C.MixedCompressor(C.TopkSparse(1.0), getattr(C, cls)(**kw)).compress(xd)


# ---------------------------------------------------------------------------
# layout edges, ties, special values: the kernels with an explicit k
# ---------------------------------------------------------------------------
_orders = {}


def _random_case(dt, n):
    """Seeded data of (dt, n) and the oracle's sort order, computed once."""
    if (dt, n) not in _orders:
        x = tc.case_input(n, (n,), 5, dt)
        keys = to.abs_key(x)
        _orders[(dt, n)] = (x, np.lexsort((np.arange(n), keys)))
    return _orders[(dt, n)]


def _kept(order, k):
    return np.sort(order[order.size - k:]).astype(np.int32)


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("n", SMALL + LARGE)
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_layout_edges(dt, n, odd):
    x, order = _random_case(dt, n)
    xd = _dev(x, misalign=odd)
    assert (xd.data_ptr() % 16 != 0) == odd
    for k in _ks(n):
        _check(xd, xd, k, _kept(order, k), x)


def _two_valued(dt, n):
    x = np.ones(n, dtype=dt)
    x[3::7] = -2.0
    x[1::2] *= -1  # signs do not matter
    return x


def _two_valued_kept(x, k):
    hi, lo = np.flatnonzero(np.abs(x) == 2), np.flatnonzero(np.abs(x) == 1)
    if k <= hi.size:
        return hi[hi.size - k:].astype(np.int32)
    return np.sort(np.concatenate([hi, lo[lo.size - (k - hi.size):]])).astype(np.int32)


@pytest.mark.parametrize("n", SMALL + LARGE)
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_ties_across_wave_and_block_boundaries(dt, n):
    tdt = _tdt(dt)
    ks = sorted(set(_ks(n)) | {n // 2, (3 * n) // 4})  # n / 2 of all-equal data: the quota ends inside a wave
    equal, zeros, two = np.full(n, -3.5, dtype=dt), np.zeros(n, dtype=dt), _two_valued(dt, n)
    zeros[::3] = -0.0
    for name, x in (("equal", equal), ("zeros", zeros), ("two", two)):
        xd = _dev(x)
        for k in ks:
            want = _two_valued_kept(x, k) if name == "two" else np.arange(n - k, n, dtype=np.int32)
            if n <= SMALL[-1]:
                assert np.array_equal(want, to.topk(x, k)[0]), (name, k)  # the closed form is the oracle's
            _check(xd, xd, k, want, x)
            if name != "zeros" and n <= LARGE[0] and 0 < k:  # sa_stc masks the complement
                sparse, res = torch.empty_like(xd), torch.empty_like(xd)
                K.stc(xd, None, None, n - k, sparse, res,
                      scratch=torch.empty(K.stc_scratch_bytes(n, tdt), dtype=torch.uint8, device=DEV))
                assert np.array_equal(np.flatnonzero(_host(sparse) != 0), want), (name, k)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_special_values(dt):
    u = np.uint32 if dt == np.float32 else np.uint64
    tiny = np.nextafter(dt(0), dt(1))
    nans = np.array([0x7FC00123, 0xFFC00456, 0x7F800001] if dt == np.float32 else
                    [0x7FF8000000000123, 0xFFF8000000000456, 0x7FF0000000000001], dtype=u).view(dt)
    sp = np.concatenate([np.array([0.0, -0.0, tiny, -tiny, 3 * tiny, np.inf, -np.inf, 1.5, -1.5], dtype=dt), nans])
    n = 1025
    x = np.resize(sp, n)
    xd = _dev(x)
    for k in (1, 3, 86, 171, 300, 512, 900, n - 1, n):
        index, data, dense = to.topk(x, k)
        _check(xd, xd, k, index, x)
    c = C.TopkSparse(0.5).compress(xd.reshape(25, 41))
    assert to.same_bits(_host(C.TopkSparse(0.5).decompress(c).reshape(-1)), to.topk(x, c.k)[2])


def test_two_runs_give_the_same_bits():
    x, order = _random_case(np.float32, LARGE[0])
    xd = _dev(x)
    k = x.size // 10
    a, b = _run(xd, xd, k), _run(xd, xd, k)
    assert all(np.array_equal(p, q) for p, q in zip(a, b)) and np.array_equal(a[0], _kept(order, k))
    r1 = C.RandomSparse(0.9, seed=5).compress(xd)
    r2 = C.RandomSparse(0.9, seed=5).compress(xd)
    assert torch.equal(r1.index, r2.index) and torch.equal(r1.compressed_data, r2.compressed_data)


def test_a_count_other_than_k_sets_the_flag():
    x, _ = _random_case(np.float32, 4 * 1024 + 3)
    xd = _dev(x)
    n, k = x.size, 400
    scratch = _scratch(n, xd.dtype)
    ibig, index = _guarded(k - 100, torch.int32, PAT_I)
    dbig, data = _guarded(k - 100, xd.dtype, PAT_F)
    flag = K.coo_flag(DEV)
    K.topk_select(xd, k, scratch)
    K.topk_fill(xd, xd, k - 100, scratch, index, data, flag)  # the select kept 400
    assert _host(flag).tolist() == [L.SA_COO_BAD_COUNT, -1]
    assert _guards_intact(ibig, k - 100, PAT_I) and _guards_intact(dbig, k - 100, PAT_F)


# ---------------------------------------------------------------------------
# RandomSparse
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 2**20 + 1])
def test_random_sparse_device_and_host_agree(n):
    seed = 0xC0FFEE_8000_0001
    for odd in (False, True):
        big = torch.zeros(n + 3, dtype=torch.int64, device=DEV)
        keys = big[1:n + 1] if odd else big[2:n + 2]
        K.topk_random_keys(seed, keys)
        got = _host(big)
        lo = 1 if odd else 2
        assert np.array_equal(got[lo:lo + n].view(np.uint64), L.topk_random_keys_host(seed, n))
        assert not got[:lo].any() and not got[lo + n:].any()
    for dt in DTYPES:
        x = tc.case_input(n, (n,), 5, dt)
        host = C.RandomSparse(0.9, seed=seed).compress(x)
        dev = C.RandomSparse(0.9, seed=seed).compress(_dev(x))
        assert dev.k == host.k == tc.keep_count(0.9, n)
        assert np.array_equal(_host(dev.index), host.index)
        assert to.same_bits(_host(dev.compressed_data), host.compressed_data)
        assert np.array_equal(host.index, to.random(x, host.k, seed)[0])
    # float32 keys select float64 data and the other way round: all four kernels
    x32, order = _random_case(np.float32, 4 * 1024 + 3)
    x64 = tc.case_input(1, (x32.size,), 5, np.float64)
    _check(_dev(x32), _dev(x64), 409, _kept(order, 409), x64)
    x64k, order64 = _random_case(np.float64, 4 * 1024 + 3)
    _check(_dev(x64k), _dev(x32), 409, _kept(order64, 409), x32)


# ---------------------------------------------------------------------------
# the sparse_mask path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_gather_against_fancy_indexing(dt):
    n = 70001
    x = tc.case_input(7, (n,), 5, dt)
    x[::5] = 0  # zeros are taken like every other value
    index = np.flatnonzero(np.random.default_rng(3).random(n) < 0.3).astype(np.int32)
    xd, idx = _dev(x), _dev(index)
    dbig, data = _guarded(index.size, _tdt(dt), PAT_F)
    flag = K.coo_flag(DEV)
    K.coo_gather(idx, xd, data, flag)
    assert _host(flag).tolist() == [0, -1] and to.same_bits(_host(data), x[index])
    assert _guards_intact(dbig, index.size, PAT_F)
    for at, bad, bit in ((17, n, L.SA_COO_BAD_RANGE), (5, -3, L.SA_COO_BAD_RANGE | L.SA_COO_BAD_ORDER),
                         (9, int(index[8]), L.SA_COO_BAD_ORDER)):
        wrong = index.copy()
        wrong[at] = bad
        data.fill_(PAT_F)
        flag = K.coo_flag(DEV)
        K.coo_gather(_dev(wrong), xd, data, flag)
        f = _host(flag).tolist()
        assert f[0] & bit == bit and f[1] == at, (at, f)
        got = _host(data)
        ok = np.ones(index.size, dtype=bool)
        ok[at] = bool(0 <= bad < n)
        assert to.same_bits(got[ok], x[wrong[ok]]) and _guards_intact(dbig, index.size, PAT_F)
        if not ok[at]:
            assert got[at] == PAT_F  # an index out of range is not used
    # through the classes: the bad index stays in the payload and decompress raises
    comp = C.TopkSparse(0.9)
    x2 = _dev(x[:70000]).reshape(700, 100)
    mask = comp.compress(x2).get_sparse_mask()
    mask.index = mask.index.clone()
    mask.index[-1] = 70000
    c = comp.compress(x2, sparse_mask=mask)
    with pytest.raises(ValueError, match=r"sparse payload \[0\]: an index lies outside the tensor's 70000 elements"):
        comp.decompress(c)


# ---------------------------------------------------------------------------
# no hidden work
# ---------------------------------------------------------------------------
def test_compress_never_synchronises():
    x = _dev(tc.case_input(11, (2**16 + 3,), 5, np.float32)).reshape(-1)
    topk, rnd = C.TopkSparse(0.9), C.RandomSparse(0.9, seed=1)
    warm = topk.compress(x)  # the scratch exists
    mask = warm.get_sparse_mask()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = topk.compress(x)
        b = rnd.compress(x)
        c = topk.compress(x, sparse_mask=mask)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(a.index, warm.index) and torch.equal(c.compressed_data, warm.compressed_data)
    assert b.k == a.k and a.nbytes == a.k * 8
    coo = a.to_coo()
    assert coo.index is a.index and coo.data is a.compressed_data and coo.is_device
