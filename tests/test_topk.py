"""TopkSparse, RandomSparse, MixedCompressor and get() on the host
(sfl_amd/utils/sparse_compressor.py, the numpy form): bit for bit against what
the reference's own classes gave (tests/golden/topk_reference.npz, made by
tests/golden/make_topk_golden.py), the reference's own round-trip contract,
the tie rule, special values, the edges of k, and RandomSparse's keys and
uniformity."""
import logging

import numpy as np
import pytest

import topk_cases as tc
import topk_oracle as to
from oracle import dp
from sfl_amd import _lib as L
from sfl_amd.utils import compressor as C
from sfl_amd.utils import sparse_compressor as SC

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def golden():
    return tc.Golden()


# ---------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(tc.SHAPES)))
def test_topk_is_the_reference_bit_for_bit(golden, si):
    cases = [c for c in tc.all_cases() if c[1] == si]
    assert len(cases) == len(tc.RATES) * len(tc.DTYPES)
    for k, _, ri, dt in cases:
        x = tc.case_input(golden.seed(k), tc.SHAPES[si], tc.scale_of(ri), dt)
        comp = C.TopkSparse(tc.RATES[ri])
        c = comp.compress(x)
        assert isinstance(c, C.SparseCompressedData) and c.k == golden.k(k), k
        assert c.index.dtype == np.int32 and np.all(np.diff(c.index) > 0), k
        assert c.origin_shape == x.shape and len(c.shape) == 2 and c.nbytes == c.k * (4 + x.itemsize), k
        dec = comp.decompress(c)
        assert dec.dtype == x.dtype and dec.shape == x.shape, k
        assert np.array_equal(tc.digest(dec), golden.dec(k)), k
        assert to.same_bits(dec, to.topk(x, c.k)[2]), k
        dec2 = comp.decompress(comp.compress(x, sparse_mask=c.get_sparse_mask()))
        assert np.array_equal(tc.digest(dec2), golden.dec_mask(k)), k
        assert to.same_bits(c.to_dense_numpy(), dec), k


@pytest.mark.parametrize("scheme", list(tc.MIXED))
def test_mixed_is_the_reference_bit_for_bit(golden, scheme):
    cls, kw = tc.MIXED[scheme]
    for k, _, si, dt in (c for c in tc.mixed_cases() if c[1] == scheme):
        x = tc.case_input(golden.seed(k), tc.SHAPES[si], tc.SCALES[1], dt)
        comp = C.MixedCompressor(C.TopkSparse(tc.MIXED_RATE), getattr(C, cls)(**kw))
        c = comp.compress(x)
        assert isinstance(c, C.MixedCompressedData), k
        assert [p.compressed_data for p in c.compressed_participants] == [None, None], k
        want = golden.codes(k)
        assert c.compressed_data.dtype == want.dtype and np.array_equal(c.compressed_data, want), k
        assert c.nbytes == 5 * golden.k(k), k
        dec = comp.decompress(c)
        assert dec.dtype == x.dtype and dec.shape == x.shape, k
        assert np.array_equal(tc.digest(dec), golden.dec(k)), k


# ---------------------------------------------------------------------------
# the reference's own checks (tests/utils/test_compressor.py:44-74, 103-111)
# ---------------------------------------------------------------------------
SHAPES = ((10, 10), (10, 10, 10), (10, 10, 10, 10))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("make", [lambda: C.TopkSparse(0.9), lambda: C.RandomSparse(0.9)], ids=["topk", "random"])
def test_the_references_sparse_round_trip(make, shape):
    comp = make()
    data = np.random.default_rng(len(shape)).uniform(low=-5, high=5, size=shape)
    c = comp.compress(data)
    assert isinstance(c, C.SparseCompressedData) and isinstance(c, C.CompressedData)
    assert comp.iscompressed(c) and comp.iscompressed([c, data]) == [True, False]
    plain = comp.decompress(c)
    c2 = comp.compress(data, sparse_mask=c.get_sparse_mask())
    assert to.same_bits(plain, comp.decompress(c2))
    assert np.array_equal(c.row * c.shape[1] + c.col, c.index) and c.row.dtype == np.int64
    assert comp.compress([data, data])[1].k == c.k and comp.decompress([c])[0].shape == shape


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("make", [lambda: C.MixedCompressor(C.TopkSparse(0.9), C.QuantizedZeroPoint()),
                                  lambda: C.MixedCompressor(C.RandomSparse(0.8), C.QuantizedLSTM())],
                         ids=["topk+zp", "random+lstm"])
def test_the_references_mixed_round_trip(make, shape):
    comp = make()
    data = np.random.default_rng(7 + len(shape)).uniform(low=-5, high=5, size=shape)
    c = comp.compress(data)
    assert isinstance(c, C.MixedCompressedData) and comp.iscompressed(c)
    plain = comp.decompress(c)
    assert plain.shape == shape and plain.dtype == data.dtype
    kept = plain != 0
    assert np.allclose(plain[kept], data[kept], atol=0.2)
    c2 = comp.compress(data, sparse_mask=c.get_sparse_mask())
    assert to.same_bits(plain, comp.decompress(c2))


def test_the_mask_keeps_zeros_in_the_data():
    x = np.arange(12, dtype=np.float32).reshape(3, 4)
    mask = C.TopkSparse(0.0).compress(x).get_sparse_mask()
    assert mask.dtype == bool and mask.shape == (3, 4) and mask.nnz == 12
    c = C.TopkSparse(0.5).compress(x, sparse_mask=mask)  # x[0, 0] == 0 is taken like every other value
    assert c.k == 12 and to.same_bits(c.compressed_data, x.reshape(-1))
    with pytest.raises(ValueError, match=r"the mask is \(3, 4\), the data \(4, 3\)"):
        C.TopkSparse(0.5).compress(x.reshape(4, 3), sparse_mask=mask)
    with pytest.raises(TypeError, match="sparse_mask"):
        C.TopkSparse(0.5).compress(x, sparse_mask=np.ones((3, 4), bool))


# ---------------------------------------------------------------------------
# ties, special values, the edges of k, shapes
# ---------------------------------------------------------------------------
def stc_support(x, rate):
    sparse = C.stc_step(x, None, None, rate)[0]
    return np.flatnonzero(np.asarray(sparse).reshape(-1) != 0)


def test_ties_keep_the_higher_indices_and_agree_with_stc():
    two = np.array([[1, -1, 1, 2], [1, 1, -1, .5]], dtype=np.float32)
    c = C.TopkSparse(0.5).compress(two)
    assert c.k == 4 and c.index.tolist() == [3, 4, 5, 6]  # the 2, then the three 1s of highest index
    assert C.mask_count(0.5, 8) == 8 - c.k and stc_support(two, 0.5).tolist() == c.index.tolist()
    for dt in (np.float32, np.float64):
        ones = np.full((5, 8), -3.5, dtype=dt)
        c = C.TopkSparse(0.75).compress(ones)
        assert c.k == 10 and c.index.tolist() == list(range(30, 40))
        assert stc_support(ones, 0.75).tolist() == c.index.tolist()
        zeros = np.zeros((5, 8), dtype=dt)
        zeros[0, 0] = -0.0
        c = C.TopkSparse(0.75).compress(zeros)
        assert c.index.tolist() == list(range(30, 40)) and not c.compressed_data.any()
        assert to.same_bits(C.TopkSparse(0.75).decompress(c), np.zeros((5, 8), dtype=dt))


@pytest.mark.parametrize("dt", tc.DTYPES)
def test_nan_inf_denormals_and_negative_zero(dt):
    tiny = np.finfo(dt).smallest_subnormal
    x = np.array([0.0, -0.0, tiny, -tiny, 1.0, -np.inf, np.nan, np.inf, -np.nan, 2 * tiny, 3.0, -1.0], dtype=dt)
    order = [8, 6, 7, 5, 10, 11, 4, 9, 3, 2, 1, 0]  # NaN first, then inf, ...; of equals the higher index first
    for k in range(len(x) + 1):
        c = C.TopkSparse(1 - k / len(x)).compress(x)
        assert c.k == k
        assert sorted(c.index.tolist()) == sorted(order[:k]), k
        assert to.same_bits(c.compressed_data, x[np.sort(order[:k]).astype(int)] if k else x[:0]), k
        assert to.same_bits(C.TopkSparse(0.5).decompress(c), to.topk(x, k)[2]), k


def test_k_of_0_1_n_minus_1_and_n():
    x = tc.case_input(3, (10, 10), 5, np.float32)
    for rate, k in ((1.0, 0), (0.99, 1), (0.01, 99), (0.0, 100)):
        for comp in (C.TopkSparse(rate), C.RandomSparse(rate, seed=11)):
            c = comp.compress(x)
            assert c.k == k and c.compressed_data.shape == (k,) and c.index.shape == (k,)
            dec = comp.decompress(c)
            assert np.count_nonzero(dec) == k and dec.shape == x.shape
            if k == 100:
                assert to.same_bits(dec, x)
        assert to.same_bits(C.TopkSparse(rate).decompress(C.TopkSparse(rate).compress(x)), to.topk(x, k)[2])
    c = C.TopkSparse(0.99).compress(x)
    assert c.index[0] == np.argmax(np.abs(x))


def test_1d_0d_and_empty_inputs():
    x = tc.case_input(5, (300,), 5, np.float64)
    c = C.TopkSparse(0.9).compress(x)
    assert c.shape == (1, 300) and c.origin_shape == (300,) and c.k == 30
    assert to.same_bits(C.TopkSparse(0.9).decompress(c), to.topk(x, 30)[2])
    s = np.array(2.5, dtype=np.float32)
    for comp in (C.TopkSparse(0.9), C.RandomSparse(0.9), C.MixedCompressor(C.TopkSparse(0.9), C.QuantizedLSTM())):
        out = comp.compress(s)
        assert out is s and comp.decompress(out) is s and not comp.iscompressed(out)
    e = C.TopkSparse(0.5).compress(np.zeros((0, 4), dtype=np.float32))
    assert e.k == 0 and C.TopkSparse(0.5).decompress(e).shape == (0, 4)
    with pytest.raises(TypeError, match="float32 or float64"):
        C.TopkSparse(0.5).compress(np.arange(8))
    with pytest.raises(TypeError, match="invalid data"):
        C.TopkSparse(0.5).compress("x")
    with pytest.raises(AssertionError):
        C.TopkSparse(1.5)


def test_cpu_tensors_come_back_as_cpu_tensors():
    x = torch.from_numpy(tc.case_input(9, (7, 33), 5, np.float32))
    for comp in (C.TopkSparse(0.9), C.RandomSparse(0.9, seed=3),
                 C.MixedCompressor(C.TopkSparse(0.9), C.QuantizedZeroPoint())):
        c = comp.compress(x)
        dec = comp.decompress(c)
        assert isinstance(dec, torch.Tensor) and not dec.is_cuda and dec.dtype == x.dtype and dec.shape == x.shape
        again = comp.decompress(comp.compress(x, sparse_mask=c.get_sparse_mask()))
        assert isinstance(again, torch.Tensor) and to.same_bits(again.numpy(), dec.numpy())
    c = C.TopkSparse(0.9).compress(x)
    assert isinstance(c.index, torch.Tensor) and c.index.dtype == torch.int32 and c.row.dtype == torch.int64
    assert to.same_bits(C.TopkSparse(0.9).decompress(c).numpy(), to.topk(x.numpy(), c.k)[2])
    host = c.to("cpu")
    assert isinstance(host.index, np.ndarray) and to.same_bits(host.to_dense(), to.topk(x.numpy(), c.k)[2])


def test_decompress_validates_a_foreign_payload():
    x = tc.case_input(9, (7, 33), 5, np.float32)
    comp = C.TopkSparse(0.9)
    for bad, why in ((231, "outside the tensor's 231 elements"), (-1, "outside the tensor's 231 elements"),
                     (None, "not strictly ascending")):
        c = comp.compress(x)
        if bad is None:
            c.index[3] = c.index[2]
        else:
            c.index[-1 if bad > 0 else 0] = bad
        with pytest.raises(ValueError, match=r"sparse payload \[1\]: .*" + why):
            comp.decompress([comp.compress(x), c])


def test_to_coo_goes_into_the_sparse_aggregator():
    from sfl_amd.device import PYU, PYUObject
    from sfl_amd.security import SparsePlainAggregator

    xs = [tc.case_input(40 + p, (7, 33), 5, np.float32) for p in range(3)]
    comp = C.TopkSparse(0.9)
    payloads = [comp.compress(x) for x in xs]
    coos = [c.to_coo() for c in payloads]
    assert all(isinstance(c, C.SparseCOO) and c.index is p.index and c.data is p.compressed_data
               for c, p in zip(coos, payloads))
    agg = SparsePlainAggregator(PYU("server", None))
    got = agg.average([PYUObject(PYU(f"p{i}", None), [c]) for i, c in enumerate(coos)], axis=0).data[0]
    want = agg.average([PYUObject(PYU(f"p{i}", None), [comp.decompress(p)]) for i, p in enumerate(payloads)],
                       axis=0).data[0]
    assert to.same_bits(np.asarray(got), np.asarray(want))
    assert C.payload_nbytes(coos) == sum(p.nbytes for p in payloads)


# ---------------------------------------------------------------------------
# get() and MixedCompressor's arguments
# ---------------------------------------------------------------------------
def test_get_builds_every_name():
    for name, params, cls in (("random_sparse", dict(sparse_rate=0.5), C.RandomSparse),
                              ("topk_sparse", dict(sparse_rate=0.5), C.TopkSparse),
                              ("stc_sparse", dict(sparse_rate=0.5), C.STCSparse),
                              ("scr_sparse", dict(threshold=0.5), C.SCRSparse),
                              ("quantized_fp", dict(quant_bits=8, format="E5M2"), C.QuantizedFP),
                              ("quantized_lstm", dict(quant_bits=8), C.QuantizedLSTM),
                              ("quantized_zeropoint", {}, C.QuantizedZeroPoint)):
        assert type(C.get(name, params)) is cls, name
    assert C.get("quantized_fp", dict(format="E5M2")).format == "E5M2"
    mixed = C.get("mixed_compressor", [dict(name="topk_sparse", params=dict(sparse_rate=0.9)),
                                       dict(name="quantized_zeropoint", params=dict(quant_bits=8))])
    assert isinstance(mixed, C.MixedCompressor) and mixed.comressors[0].sparse_rate == 0.9
    with pytest.raises(ValueError, match="quantized_kmeans.*not built"):
        C.get("quantized_kmeans", {})
    with pytest.raises(ValueError, match="Compressor 'nope' not exists"):
        C.get("nope", {})
    assert C.get is SC.get


def test_mixed_compressor_checks_its_arguments(caplog):
    with caplog.at_level(logging.WARNING):
        m = C.MixedCompressor(C.QuantizedLSTM(), C.TopkSparse(0.9))
    assert isinstance(m.comressors[0], C.TopkSparse) and isinstance(m.comressors[1], C.QuantizedLSTM)
    assert "first use sparse compress" in caplog.text
    for bad in ((C.TopkSparse(0.9), C.TopkSparse(0.9)), (C.QuantizedLSTM(), C.QuantizedLSTM()),
                (C.TopkSparse(0.9), C.STCSparse(0.9))):
        with pytest.raises(RuntimeError, match="Only support 2 compressors"):
            C.MixedCompressor(*bad)
    for bad in ((C.TopkSparse(0.9),), (C.TopkSparse(0.9), C.QuantizedLSTM(), C.QuantizedLSTM())):
        with pytest.raises(AssertionError, match="Only support 2 compressors"):
            C.MixedCompressor(*bad)
    with pytest.raises(ValueError, match=r"mixed entry \[1\]: the sparse payload is empty"):
        # k = round(0.1 * 100) = 10, then round(0.1 * 4) = 0
        C.MixedCompressor(C.TopkSparse(0.9), C.QuantizedLSTM()).compress(
            [tc.case_input(1, (10, 10), 5, np.float32), np.ones((2, 2), dtype=np.float32)])


# ---------------------------------------------------------------------------
# RandomSparse
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 0x1_0000_0000, 0xDEADBEEF_80000001, 2**64 - 1])
@pytest.mark.parametrize("n", [1, 2, 7, 64, 1001])
def test_the_host_keys_are_the_philox_words(seed, n):
    keys = L.topk_random_keys_host(seed, n)
    w = dp.philox_words(seed, 0, 2 * n).reshape(-1).astype(np.uint64)
    want = ((w[1:2 * n:2] << np.uint64(32)) | w[0:2 * n:2]) >> np.uint64(1)
    assert keys.dtype == np.uint64 and np.array_equal(keys, want)
    assert np.array_equal(keys, to.random_keys(seed, n)) and not np.any(keys >> np.uint64(63))
    if n > 2:  # a longer stream starts with the shorter one
        assert np.array_equal(L.topk_random_keys_host(seed, n - 1), keys[:-1])


def test_random_sparse_keeps_k_entries_of_x_reproducibly():
    x = tc.case_input(21, (10, 10, 10), 5, np.float64)
    a, b = C.RandomSparse(0.9, seed=0x1_2345_6789), C.RandomSparse(0.9, seed=0x1_2345_6789)
    ca, cb = a.compress(x), b.compress(x)
    assert ca.k == 100 and np.all(np.diff(ca.index) > 0) and 0 <= ca.index[0] and ca.index[-1] < 1000
    assert to.same_bits(ca.compressed_data, x.reshape(-1)[ca.index])
    assert np.array_equal(ca.index, cb.index)
    assert np.array_equal(ca.index, to.random(x, 100, 0x1_2345_6789)[0])
    ca2 = a.compress(x)  # the next draw: seed + 1
    assert (a.seed, a.draws) == (0x1_2345_6789, 2) and not np.array_equal(ca2.index, ca.index)
    assert np.array_equal(ca2.index, to.random(x, 100, 0x1_2345_678A)[0])
    lst = b.compress([x, x])
    assert np.array_equal(lst[0].index, ca2.index) and not np.array_equal(lst[1].index, lst[0].index)
    a.compress(x, sparse_mask=ca.get_sparse_mask())
    assert a.draws == 2  # a mask draws nothing
    fresh = C.RandomSparse(0.9)
    assert 0 <= fresh.seed < 2**64 and fresh.seed != C.RandomSparse(0.9).seed
    wrap = C.RandomSparse(0.9, seed=2**64 - 1)
    wrap.compress(x)
    assert np.array_equal(wrap.compress(x).index, to.random(x, 100, 0)[0])  # seed + 1 mod 2^64


def test_random_sparse_is_uniform():
    """n = 64, k = 16, 2000 seeds: the inclusion counts c have mean e = 500;
    sum((c - e)^2) / (e (1 - p)) * (n - 1) / n with p = 1/4 is chi-square with
    63 degrees of freedom (sampling without replacement: the counts' variance
    is e (1 - p), their sum is fixed).  [23.16, 131.37] are its 1e-6 and
    1 - 1e-6 quantiles; the numpy oracle of the definition gives 67.84 on these
    seeds.  Deterministic."""
    n, k, seeds = 64, 16, 2000
    x = np.arange(n, dtype=np.float32).reshape(8, 8)
    count = np.zeros(n, dtype=np.int64)
    for s in range(seeds):
        c = C.RandomSparse(0.75, seed=0x5EED0000 + s).compress(x)
        assert c.k == k
        count[c.index] += 1
    e, p = seeds * k / n, k / n
    stat = float(np.sum((count - e) ** 2) / (e * (1 - p)) * (n - 1) / n)
    print(f"uniformity statistic {stat:.2f}")
    assert 23.16 < stat < 131.37, stat
    assert abs(stat - 67.84) < 0.005  # the oracle's figure: host path and definition agree
