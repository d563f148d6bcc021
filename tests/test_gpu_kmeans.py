"""QuantizedKmeans on the GPU (sa_kmeans_hist / _step / _labels and
sa_dequant_lut) against the numpy form (sfl_amd/utils/quantized.py on host
arrays, itself pinned to the plain-integer oracle by tests/test_kmeans_host.py):
bit for bit in codes, ``q`` and ``n_iter``."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import kmeans_cases as kc  # noqa: E402
from gpu_copies import DEV, _bits, _dev, _host  # noqa: E402

from sfl_amd.utils import quantized as Q  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = (np.float32, np.float64)
IDS = ["f32", "f64"]
# K + 1: the smallest tensor that is clustered; 255 .. 257: around one block's
# 256 threads and the code kernel's runs of 16; 1023: one tile of the wave
# layout short of a block's four; 4100: several blocks; 70,003: 69 blocks and
# a ragged last wave
N = (255, 256, 257, 1023, 4100, 70_003)
# (K, quant_bits): 2 and 8 search 1 and 3 probes with 64 table copies, 256
# searches 8 probes with 4 copies; int16 codes at 16 bits
KB = ((2, 8), (8, 8), (256, 8), (256, 16))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _data(n, dt, seed=0):
    """Two normal clumps of unequal width: every step moves centres for a while."""
    rng = np.random.default_rng(1000 * seed + n)
    return np.where(rng.random(n) < 0.3, rng.standard_normal(n) * 0.2 - 2.0, rng.standard_normal(n)).astype(dt)


def _both(x, xd, **kw):
    """The payload of the host array ``x`` and of the device tensor ``xd``."""
    km = Q.QuantizedKmeans(**kw)
    return km, km.compress(x), km.compress(xd)


def _same_payload(h, d):
    assert d.is_device and d.compressed_data.dtype == Q._torch_dtype(h.compressed_data.dtype)
    assert d.compressed_data.shape == h.compressed_data.shape
    assert (d.n_iter, d.quant_bits, d.origin_type) == (h.n_iter, h.quant_bits, h.origin_type)
    assert isinstance(d.q, np.ndarray) and d.q.shape == h.q.shape and d.q.dtype == h.q.dtype
    assert np.array_equal(_bits(d.q), _bits(h.q))
    assert np.array_equal(_host(d.compressed_data), h.compressed_data)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("kb", KB, ids=lambda kb: f"k{kb[0]}b{kb[1]}")
def test_the_device_form_is_the_numpy_form_bit_for_bit(kb, dt):
    K, bits = kb
    for n in (K + 1,) + N:
        if n <= K:
            continue
        x = _data(n, dt)
        km, h, d = _both(x, _dev(x), quant_bits=bits, n_clusters=K, init="cbrt", max_iter=6)
        _same_payload(h, d)
        assert h.compressed_data.dtype == (np.int8 if bits == 8 else np.int16)
        dec = km.decompress(d)
        assert dec.is_cuda and np.array_equal(_bits(_host(dec)), _bits(km.decompress(h)))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_a_view_offset_by_one_element_takes_the_unaligned_path(dt):
    for n in (257, 4100):
        x = _data(n, dt, seed=1)
        km, h, d = _both(x, _dev(x, misalign=True), quant_bits=8, n_clusters=8, init="cbrt", max_iter=6)
        _same_payload(h, d)
        # the codes offset by one element too: the decoder's scalar head
        big = torch.empty(n + 1, dtype=d.compressed_data.dtype, device=DEV)
        big[1:].copy_(d.compressed_data)
        d.compressed_data = big[1:]
        assert np.array_equal(_bits(_host(km.decompress(d))), _bits(km.decompress(h)))


@pytest.mark.parametrize("name", sorted(kc.POSITIONED))
def test_decisive_elements_at_every_kind_of_position(name):
    """The element on a boundary and the half-way mean (kmeans_cases.py), with
    the decisive element in the scalar head, a lane's first and last slot,
    either side of a block's edge and in the tail."""
    n = 1000
    for pos in (0, 3, 4, 255, 256, n - 2, n - 1):
        case = kc.POSITIONED[name](n, pos)
        km, h, d = _both(case["x"], _dev(case["x"]), quant_bits=8, n_clusters=case["K"], init=case["init"],
                         max_iter=case["max_iter"])
        _same_payload(h, d)
        assert d.n_iter == case["n_iter"]
        assert int(_host(d.compressed_data)[case["probe"]]) + 128 == case["label"], pos


@pytest.mark.parametrize("name", sorted(kc.SMALL) + ["sum53"])
def test_decisive_sums_counts_and_stops(name):
    """A sum beyond 32 bits, a sum beyond 2^53, an empty cluster and the step count (kmeans_cases.py)."""
    case = kc.sum53() if name == "sum53" else kc.SMALL[name]()
    km, h, d = _both(case["x"], _dev(case["x"]), quant_bits=8, n_clusters=case["K"], init=case["init"],
                     max_iter=case["max_iter"])
    _same_payload(h, d)
    assert d.n_iter == case["n_iter"]
    assert int(_host(d.compressed_data)[case["probe"]]) + 128 == case["label"]


def test_a_converged_fit_freezes_the_state():
    """The clumps converge in 2 steps; the 48 steps enqueued behind them find
    ``done`` set and change nothing."""
    x = kc.data("clumps", np.float32)
    km, h, d = _both(x, _dev(x), quant_bits=8, init="cbrt", max_iter=50)
    assert h.n_iter == 2
    _same_payload(h, d)


def test_the_same_bits_twice_over_dirty_scratch():
    from sfl_amd.utils import compressor as C

    x = _data(70_003, np.float32, seed=2)
    xd = _dev(x)
    km = Q.QuantizedKmeans(8, 64, init="cbrt", max_iter=8)
    runs = []
    for _ in range(2):
        for s in C._scratch.values():
            s.fill_(0xFF)
        d = km.compress(xd)
        runs.append((_host(d.compressed_data), d.q, d.n_iter))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(_bits(runs[0][1]), _bits(runs[1][1]))
    assert runs[0][2] == runs[1][2]
    _same_payload(km.compress(x), d)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("store", (np.int8, np.int16), ids=("i8", "i16"))
def test_the_lut_decoder_and_its_flag(store, dt):
    """sa_dequant_lut against ``q[label]``; a code outside the clusters at the
    first, a middle and the last position raises with the least position."""
    from sfl_amd import kernels as Kn

    bits = 8 if store == np.int8 else 16
    half, K, n = 1 << (bits - 1), 200, 4099
    rng = np.random.default_rng(5)
    q = np.sort(rng.standard_normal(K)).astype(dt)
    codes = (rng.integers(0, K, n) - half).astype(store)
    out = torch.empty(n, dtype=Q._torch_dtype(np.dtype(dt)), device=DEV)
    flag = Kn.coo_flag(DEV)
    Kn.dequant_lut(_dev(codes), _dev(q), half, out, flag)
    assert np.array_equal(_bits(_host(out)), _bits(q[codes.astype(np.int64) + half]))
    assert [int(v) for v in _host(flag).view(np.uint32)] == [0, 0xFFFFFFFF]
    km = Q.QuantizedKmeans(bits, K, init="cbrt")
    for where in ((0,), (n // 2, n - 1), (n - 1,), (7, 0, n - 1)):
        wrong = codes.copy()
        wrong[list(where)] = K - half  # the label K: the first one outside
        payload = Q.KmeansCompressData(_dev(wrong), bits, np.dtype(dt), q.reshape(-1, 1), 1)
        with pytest.raises(ValueError, match=rf"outside the {K} clusters at position {min(where)}$"):
            km.decompress(payload)


def test_a_negative_label_is_flagged_too():
    """At 4 bits the int8 code -9 is the label -1."""
    q = np.arange(10, dtype=np.float32).reshape(-1, 1)
    codes = (np.arange(300) % 10 - 8).astype(np.int8)
    km = Q.QuantizedKmeans(4, 10, init="cbrt")
    good = km.decompress(Q.KmeansCompressData(_dev(codes), 4, np.dtype(np.float32), q, 1))
    assert np.array_equal(_host(good), (np.arange(300) % 10).astype(np.float32))
    codes[123] = -9
    with pytest.raises(ValueError, match=r"at position 123$"):
        km.decompress(Q.KmeansCompressData(_dev(codes), 4, np.dtype(np.float32), q, 1))


def test_refusals_and_the_mixed_compressor_on_the_device():
    from sfl_amd.utils import compressor as C

    x = _data(5000, np.float32, seed=3)
    km = Q.QuantizedKmeans(8, init="cbrt")
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[17] = bad
        with pytest.raises(ValueError, match="quantized entry"):
            km.compress(_dev(y))
    with pytest.raises(ValueError, match="quantized entry"):
        km.compress(_dev(np.full(100, 2.5, dtype=np.float32)))
    with pytest.raises(ValueError, match="n_clusters <= 256"):
        Q.QuantizedKmeans(16, 257, init="cbrt").compress(_dev(x))
    small = _dev(x[:8])
    assert km.compress(small).compressed_data is small  # n <= K passes through
    mixed = C.MixedCompressor(C.TopkSparse(0.9), Q.QuantizedKmeans(8, init="cbrt"))
    md, mh = mixed.compress(_dev(x).reshape(50, 100)), mixed.compress(x.reshape(50, 100))
    assert md.is_device and np.array_equal(_host(md.compressed_data), mh.compressed_data)
    assert np.array_equal(_bits(_host(mixed.decompress(md))), _bits(mixed.decompress(mh)))
