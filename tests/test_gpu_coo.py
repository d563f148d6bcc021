"""The sa_coo kernels on the GPU against the numpy restatement
(tests/coo_oracle.py), bit for bit: the two-pass encode, the validated
decode, what a malformed payload does, and the device form of
``sparse_encode`` / ``sparse_decode`` / ``SparseCOO.to``.  Every output is a
view into a larger allocation whose 64 guard elements on both sides must come
back unchanged."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import coo_oracle as co  # noqa: E402
from gpu_copies import DEV, _bits, _dev, _host  # noqa: E402

pytestmark = pytest.mark.gpu
# 65,537: 257 waves, the last block part empty; 2^20 + 3: the first n with two tiles per wave
N = (1, 3, 4, 5, 255, 256, 257, 511, 513, 1023, 1025, 65537, 2**20 + 3, 3 * 2**20 + 5)
DTYPES = (np.float32, np.float64)
IDS = ["f32", "f64"]
GUARD = 64
PAT_F, PAT_I = 12345.0, -77


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _tdt(dt):
    return torch.float32 if np.dtype(dt) == np.float32 else torch.float64


def _specials(dt):
    """+-0, the least denormal of either sign, +-inf, NaNs of both signs with payload bits."""
    u = np.uint32 if dt == np.float32 else np.uint64
    tiny = np.nextafter(dt(0), dt(1))
    nans = np.array([0x7FC00123, 0xFFC00456, 0x7F800001] if dt == np.float32 else
                    [0x7FF8000000000123, 0xFFF8000000000456, 0x7FF0000000000001], dtype=u).view(dt)
    return np.concatenate([np.array([0.0, -0.0, tiny, -tiny, np.inf, -np.inf, 1.5, -0.0], dtype=dt), nans])


def _patterns(dt, n):
    """name -> flat array of n elements."""
    rng = np.random.default_rng(n)
    v = (rng.standard_normal(n) + 3.0).astype(dt)  # no zero among them
    out = {"zero": np.zeros(n, dt), "full": v.copy()}
    for name, at in (("first", 0), ("last", n - 1)):
        x = np.zeros(n, dt)
        x[at] = -2.5
        out[name] = x
    edges = np.zeros(n, dt)  # lane 63's last and lane 0's first element of every tile of 256
    edges[255::256] = v[255::256]
    edges[0::256] = v[0::256]
    out["edges"] = edges
    for dens in (0.01, 0.5):
        out[f"rand{dens}"] = np.where(rng.random(n) < dens, v, dt(0))
    sp = _specials(dt)
    x = np.resize(sp, n)
    if n > 64:
        x = np.where(rng.random(n) < 0.3, x, dt(0))
    out["special"] = x
    return out


_cases = {}


def _case(dt, n):
    """The patterns of (dt, n) with the oracle's encoding, computed once."""
    if (dt, n) not in _cases:
        _cases[(dt, n)] = {name: (x, *co.encode(x)) for name, x in _patterns(dt, n).items()}
    return _cases[(dt, n)]


def _guarded(n, tdt, fill, odd=False):
    """(the whole allocation, the view of n elements inside it); ``odd``: the
    view starts one element further, so it is element-aligned only."""
    lo = GUARD + (1 if odd else 0)
    big = torch.full((lo + n + GUARD,), fill, dtype=tdt, device=DEV)
    return big, big[lo:lo + n], lo


def _guards_intact(big, lo, n, fill):
    h = _host(big)
    return bool(np.all(h[:lo] == fill) and np.all(h[lo + n:] == fill))


def _encode(x, misalign=False, garbage=0x5A5A5A5A, cap=None):
    """count + fill on the device: (nnz, index, data, flag bits, guards intact)."""
    from sfl_amd import kernels as K

    tx = _dev(x, misalign)
    tdt = tx.dtype
    words = K.coo_scratch_bytes(x.size, tdt) // 4
    scratch = torch.full((words,), garbage - (1 << 32) if garbage >= 1 << 31 else garbage, dtype=torch.int32,
                         device=DEV)
    count = torch.full((1,), -5, dtype=torch.int32, device=DEV)
    K.coo_count(tx, scratch, count)
    nnz = int(_host(count)[0])
    m = nnz if cap is None else cap
    ibig, index, ilo = _guarded(m, torch.int32, PAT_I)
    dbig, data, dlo = _guarded(m, tdt, PAT_F, odd=misalign)
    flag = K.coo_flag(DEV)
    K.coo_fill(tx, scratch, index, data, flag)
    torch.cuda.synchronize()
    ok = _guards_intact(ibig, ilo, m, PAT_I) and _guards_intact(dbig, dlo, m, PAT_F)
    return nnz, _host(index), _host(data), _host(flag), ok


def _decode(idx, data, n, dt, misalign=False):
    """(dense, flag record, guards intact) of a payload onto a dense_out that held garbage."""
    from sfl_amd import kernels as K

    big, dense, lo = _guarded(n, _tdt(dt), PAT_F, odd=misalign)
    flag = K.coo_flag(DEV)
    K.coo_decode(_dev(np.asarray(idx, np.int32)), _dev(np.asarray(data, dt)), dense, flag)
    torch.cuda.synchronize()
    return _host(dense), _host(flag), _guards_intact(big, lo, n, PAT_F)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", N)
def test_encode_matches_the_restatement(dt, n):
    for name, (x, ridx, rdata) in _case(dt, n).items():
        for misalign in ((False, True) if name.startswith("rand") else (False,)):
            nnz, index, data, flag, ok = _encode(x, misalign)
            what = (name, misalign)
            assert nnz == ridx.size, what
            assert index.dtype == np.int32 and np.array_equal(index, ridx), what
            assert data.dtype == x.dtype and np.array_equal(_bits(data), _bits(rdata)), what
            assert flag.tolist() == [0, -1] and ok, what


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", N)
def test_decode_and_round_trip(dt, n):
    for name, (x, ridx, rdata) in _case(dt, n).items():
        for misalign in ((False, True) if name.startswith("rand") else (False,)):
            dense, flag, ok = _decode(ridx, rdata, n, dt, misalign)
            what = (name, misalign)
            assert np.array_equal(_bits(dense), _bits(co.decode(ridx, rdata, (n,), dt))), what
            assert flag.tolist() == [0, -1] and ok, what
            # decode(encode(x)) == x, except that -0.0 became +0.0
            want = np.where(co.nonzero_mask(x), x, dt(0))
            assert np.array_equal(_bits(dense), _bits(want)), what


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", (5, 1025, 65537, 2**20 + 3))
def test_a_short_cap_is_reported_and_nothing_is_stored_beyond_it(dt, n):
    from sfl_amd import _lib as L

    for name in ("full", "rand0.5", "edges"):
        x, ridx, rdata = _case(dt, n)[name]
        cap = ridx.size - 1
        nnz, index, data, flag, ok = _encode(x, cap=cap)
        assert nnz == ridx.size and flag[0] == L.SA_COO_BAD_COUNT and ok, name
        assert np.array_equal(index, ridx[:cap]) and np.array_equal(_bits(data), _bits(rdata[:cap])), name


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", (257, 65537, 2**20 + 3))
def test_two_runs_give_identical_bits(dt, n):
    for name in ("rand0.5", "special"):
        x = _case(dt, n)[name][0]
        a = _encode(x, garbage=0x01234567)
        b = _encode(x, garbage=0xFEDCBA98)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[2]), _bits(b[2])), name


# ---------------------------------------------------------------------------
# malformed payloads
# ---------------------------------------------------------------------------
MAL_N, MAL_NNZ = 2000, 600


def _malformed(dt):
    """name -> (index, least offending entry, SA_COO_BAD_* bit): every offence
    at entry 0, at entry 256 and at the last entry of a payload of 600."""
    from sfl_amd import _lib as L

    good = (5 + 3 * np.arange(MAL_NNZ)).astype(np.int64)
    out = {}
    for p in (0, 256, MAL_NNZ - 1):
        for name, v in (("minus1", -1), ("n", MAL_N), ("int_min", -2**31)):
            idx = good.copy()
            idx[p] = v
            # an index out of range also breaks the order: entry p itself (too low) or entry p + 1 (too high)
            out[f"{name}@{p}"] = (idx, p if (p > 0 or v >= MAL_N) else 0, L.SA_COO_BAD_RANGE)
        dup, desc = good.copy(), good.copy()
        if p == 0:
            dup[0], desc[0] = good[1], good[1] + 1  # entry 1 is the first that offends
        else:
            dup[p], desc[p] = good[p - 1], good[p - 1] - 1
        out[f"duplicate@{p}"] = (dup, max(p, 1), L.SA_COO_BAD_ORDER)
        out[f"descent@{p}"] = (desc, max(p, 1), L.SA_COO_BAD_ORDER)
    return good.astype(np.int32), {k: (i.astype(np.int32), at, bit) for k, (i, at, bit) in out.items()}


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_malformed_payloads_set_the_flag_and_stay_inside(dt):
    from sfl_amd import kernels as K

    _, bad = _malformed(dt)
    data = np.arange(1, MAL_NNZ + 1).astype(dt)
    for name, (idx, at, bit) in bad.items():
        dense, flag, ok = _decode(idx, data, MAL_N, dt)
        assert ok, name
        assert int(flag[0]) & bit, (name, flag)
        assert int(flag[1]) == at, (name, flag)
        # the same through the server's axpy, onto an accumulator between guards
        for adt in ((torch.float32, torch.float64) if dt == np.float32 else (torch.float64,)):
            big, acc, lo = _guarded(MAL_N, adt, PAT_F)
            f = K.coo_flag(DEV)
            K.coo_axpy(_dev(idx), _dev(data), 0.5, acc, f)
            torch.cuda.synchronize()
            f = _host(f)
            assert _guards_intact(big, lo, MAL_N, PAT_F) and int(f[0]) & bit and int(f[1]) == at, (name, adt, f)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_malformed_payloads_raise_the_host_paths_words(dt):
    from sfl_amd.device import PYU, PYUObject
    from sfl_amd.security import SparsePlainAggregator
    from sfl_amd.utils.sparse import SparseCOO, sparse_decode

    good_idx, bad = _malformed(dt)
    data = np.arange(1, MAL_NNZ + 1).astype(dt)
    good = SparseCOO((MAL_N,), dt, good_idx, data)
    agg = SparsePlainAggregator(PYU("server", None))
    for name, (idx, _, _) in bad.items():
        c = SparseCOO((MAL_N,), dt, idx, data)
        with pytest.raises(ValueError) as host:
            sparse_decode([good, c])
        with pytest.raises(ValueError) as dev:
            sparse_decode([good.to(DEV), c.to(DEV)])
        assert str(dev.value) == str(host.value) and "[1]" in str(dev.value), name
        for call in ("sum", "average"):
            with pytest.raises(ValueError) as host:
                getattr(agg, call)([PYUObject(PYU("a", None), [good]), PYUObject(PYU("b", None), [c])], axis=0)
            with pytest.raises(ValueError) as dev:
                getattr(agg, call)([PYUObject(PYU("a", None), [good.to(DEV)]),
                                    PYUObject(PYU("b", None), [c.to(DEV)])], axis=0)
            assert str(dev.value) == str(host.value) and "layer 0, party 1" in str(dev.value), (name, call)


# ---------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_sparse_encode_of_a_device_tensor_stays_on_the_device(dt):
    from sfl_amd.utils.sparse import SparseCOO, payload_nbytes, sparse_decode, sparse_encode

    x = _case(dt, 1025)["rand0.5"][0][:1024].reshape(4, 16, 16)
    ridx, rdata = co.encode(x)
    tx = _dev(x).reshape(x.shape)
    (c,) = sparse_encode([tx])
    assert isinstance(c, SparseCOO) and c.shape == x.shape and c.dtype == x.dtype and c.is_device
    assert c.index.is_cuda and c.data.is_cuda and c.index.dtype == torch.int32 and c.data.dtype == tx.dtype
    assert np.array_equal(_host(c.index), ridx) and np.array_equal(_bits(_host(c.data)), _bits(rdata))
    assert c.nnz == ridx.size and c.nbytes == ridx.size * (4 + x.dtype.itemsize) == payload_nbytes([c])
    assert np.array_equal(c.coords, co.coords(x))
    (back,) = sparse_decode([c])
    assert back.is_cuda and back.shape == tx.shape and back.dtype == tx.dtype
    assert np.array_equal(_bits(_host(back)), _bits(x + 0))
    assert np.array_equal(_bits(_host(c.todense())), _bits(x + 0))
    # to the host and back
    h = c.to("cpu")
    assert isinstance(h.index, np.ndarray) and np.array_equal(h.index, ridx) and \
        np.array_equal(_bits(h.data), _bits(rdata)) and not h.is_device
    d = h.to(DEV)
    assert d.is_device and np.array_equal(_host(d.index), ridx) and np.array_equal(_bits(_host(d.data)), _bits(rdata))
    assert np.array_equal(_bits(sparse_decode([h])[0]), _bits(x + 0))
    # an all-zero and an empty tensor
    (z,) = sparse_encode([torch.zeros(7, 3, dtype=tx.dtype, device=DEV)])
    assert z.nnz == 0 and z.is_device and not _bits(_host(sparse_decode([z])[0])).any()
    (e,) = sparse_encode([torch.zeros(0, 3, dtype=tx.dtype, device=DEV)])
    assert e.nnz == 0 and sparse_decode([e])[0].shape == (0, 3)


def test_other_element_types_and_host_inputs():
    from sfl_amd.utils.sparse import sparse_decode, sparse_encode

    counter = torch.zeros((), dtype=torch.int64, device=DEV) + 7  # num_batches_tracked on a GPU model
    (c,) = sparse_encode([counter])
    assert isinstance(c.index, np.ndarray) and isinstance(c.data, np.ndarray) and not c.is_device
    assert c.dtype == np.int64 and c.shape == () and c.nnz == 1 and int(sparse_decode([c])[0]) == 7
    x = _case(np.float32, 255)["rand0.5"][0]
    (h,) = sparse_encode([x])  # a host input gives what it gave
    assert isinstance(h.index, np.ndarray) and np.array_equal(h.index, co.encode(x)[0])
    (t,) = sparse_encode([torch.from_numpy(x.copy())])
    assert isinstance(t.index, torch.Tensor) and not t.index.is_cuda and not t.is_device
    assert isinstance(sparse_decode([t])[0], torch.Tensor) and not sparse_decode([t])[0].is_cuda


def test_the_wrappers_check_their_arguments():
    from sfl_amd import kernels as K

    x = _dev(np.ones(512, np.float32))
    scratch = torch.empty(K.coo_scratch_bytes(512, torch.float32) // 4, dtype=torch.int32, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    index = torch.zeros(512, dtype=torch.int32, device=DEV)
    data = torch.zeros(512, dtype=torch.float32, device=DEV)
    flag = K.coo_flag(DEV)
    with pytest.raises(ValueError, match="device-resident"):
        K.coo_count(torch.ones(512), scratch, count)
    with pytest.raises(ValueError, match="device-resident"):
        K.coo_decode(index, data, torch.zeros(512), flag)
    with pytest.raises(TypeError):
        K.coo_count(x.to(torch.float16), scratch, count)
    with pytest.raises(TypeError):
        K.coo_scratch_bytes(512, torch.int64)
    with pytest.raises(ValueError, match="contiguous"):
        K.coo_count(x[::2], scratch, count)
    with pytest.raises(ValueError, match="scratch"):
        K.coo_count(x, scratch[:8], count)
    with pytest.raises(ValueError):
        K.coo_count(x, scratch, count.to(torch.int64))
    with pytest.raises(ValueError):
        K.coo_fill(x, scratch, index.to(torch.int64), data, flag)
    with pytest.raises(ValueError):
        K.coo_fill(x, scratch, index, data.to(torch.float64), flag)
    with pytest.raises(ValueError):
        K.coo_fill(x, scratch, index[::2], data[::2], flag)
    with pytest.raises(ValueError):
        K.coo_fill(x, scratch, index, data, flag, cap=513)
    with pytest.raises(ValueError):
        K.coo_decode(index, data[:100], torch.zeros(512, dtype=torch.float32, device=DEV), flag)
    with pytest.raises(ValueError):
        K.coo_decode(index, data, torch.zeros(100, dtype=torch.float32, device=DEV), flag)
    with pytest.raises(ValueError):
        K.coo_decode(index, data, torch.zeros(512, dtype=torch.float64, device=DEV), flag)
    with pytest.raises(TypeError):
        K.coo_axpy(index, data.to(torch.float64), 1.0, torch.zeros(512, dtype=torch.float32, device=DEV), flag)
    with pytest.raises(TypeError):
        K.coo_axpy(index, data, 1.0, torch.zeros(512, dtype=torch.int64, device=DEV), flag)
    with pytest.raises(ValueError):
        K.coo_axpy(index, data, 1.0, torch.zeros(1024, dtype=torch.float32, device=DEV)[::2], flag)
    with pytest.raises(ValueError):
        K.coo_axpy(index, data, 1.0, torch.zeros(512, dtype=torch.float32, device=DEV), flag[:1])
    with pytest.raises(TypeError):
        K.coo_finish(torch.zeros(8, dtype=torch.int64, device=DEV), 2.0)
    with pytest.raises(ValueError):
        K.coo_finish(torch.zeros(16, dtype=torch.float32, device=DEV)[::2], 2.0)
