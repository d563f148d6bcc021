"""QuantizedKmeans on host arrays (sfl_amd/utils/quantized.py, the numpy
form): its decoder against the reference's recorded payload, the fit against
the plain-integer oracle (tests/kmeans_oracle.py), its quality against the
reference's five random starts (tests/golden/kmeans_reference.npz, made by
tests/golden/make_kmeans_golden.py), the decisive elements and every refusal."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import kmeans_cases as kc  # noqa: E402
import kmeans_oracle as o  # noqa: E402

from sfl_amd.utils import compressor as C  # noqa: E402
from sfl_amd.utils import quantized as Q  # noqa: E402

DTYPES = (np.float32, np.float64)
IDS = ["f32", "f64"]


@pytest.fixture(scope="module")
def golden():
    with np.load(kc.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _oracle(x, K, init, max_iter=50, variant=None):
    """The oracle's fit of ``x`` as (labels, q in x's type, n_iter)."""
    xs = [float(v) for v in x.reshape(-1)]
    start = init if isinstance(init, str) else [float(v) for v in init]
    labels, _, n_iter, q = o.fit(xs, K, start, max_iter, variant)
    return np.array(labels), np.array(q, dtype=np.float64).astype(x.dtype).reshape(-1, 1), n_iter


def _against_oracle(x, bits, K, init, max_iter=50):
    c = Q.QuantizedKmeans(bits, K, init=init, max_iter=max_iter).compress(x)
    labels, q, n_iter = _oracle(x, K, init, max_iter)
    assert c.n_iter == n_iter
    assert c.q.dtype == x.dtype and c.q.shape == (K, 1) and np.array_equal(_bits(c.q), _bits(q))
    assert c.compressed_data.shape == x.shape
    assert np.array_equal(c.compressed_data.astype(np.int64) + (1 << (bits - 1)), labels.reshape(x.shape))
    return c


# ---------------------------------------------------------------------------
# the reference's payload and its quality
# ---------------------------------------------------------------------------
def test_decode_parity_with_the_references_payload(golden):
    """``decompress`` of a payload built from the reference's recorded codes
    and ``q`` is the reference's decompressed array, bit for bit."""
    kind, dt, K = kc.CODES_CASE
    codes, q, dec = golden["codes"], golden["q"], golden["dec"]
    assert codes.dtype == np.int8 and q.shape == (K, 1) and dec.dtype == dt
    got = Q.QuantizedKmeans(8, K, init="cbrt").decompress(Q.KmeansCompressData(codes, 8, np.dtype(dt), q))
    assert got.dtype == dec.dtype and got.shape == dec.shape
    assert np.array_equal(_bits(got), _bits(dec))


@pytest.mark.parametrize("case", kc.all_cases(), ids=lambda c: kc.key(*c))
def test_the_error_is_within_a_tenth_of_the_references_median(golden, case):
    """Our sum of squared errors is at most 1.10 times the median of the
    reference's five runs (random_state 0..4): a condition on the definition,
    not a measurement of it."""
    kind, dt, K = case
    x = kc.data(kind, dt)
    km = Q.QuantizedKmeans(8, K, init="cbrt")
    c = km.compress(x)
    ours = kc.sse(x, km.decompress(c))
    ref = float(np.median(golden["sse"][list(golden["keys"]).index(kc.key(*case))]))
    print(f"{kc.key(*case)}: ours {ours:.6g}, reference median {ref:.6g}, ratio {ours / ref:.4f}, n_iter {c.n_iter}")
    assert ours <= 1.10 * ref


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_the_clumps_converge_in_two_steps_to_their_means(dt):
    x = kc.data("clumps", dt)
    c = Q.QuantizedKmeans(8, init="cbrt").compress(x)
    assert c.n_iter == 2 and c.compressed_data.dtype == np.int8
    labels = c.compressed_data.astype(np.int64) + 128
    assert np.array_equal(labels, np.repeat(np.arange(8), 3000))
    means = np.array([np.mean(x[labels == j], dtype=np.float64) for j in range(8)])
    # the centre is the clump's mean up to a unit of the image (range * 2^-32) and T's rounding
    width = float(x.max()) - float(x.min())
    assert np.all(np.abs(c.q.reshape(-1).astype(np.float64) - means) <= width * 2.0 ** -32 + np.finfo(dt).eps * 9.05)


# ---------------------------------------------------------------------------
# the numpy form against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_the_numpy_form_is_the_oracle(dt):
    rng = np.random.default_rng(21)
    x = np.where(rng.random(3000) < 0.3, rng.standard_normal(3000) * 0.2 - 2.0, rng.standard_normal(3000)).astype(dt)
    _against_oracle(x, 8, 8, "cbrt")
    _against_oracle(x[:1200].reshape(30, 40), 4, 5, "cbrt", max_iter=7)
    _against_oracle(x[:400], 16, 16, np.sort(x[:16]), max_iter=4)  # a start given as an array
    _against_oracle(rng.laplace(size=500).astype(dt), 8, 3, "cbrt")


def test_cpu_tensors_give_cpu_tensors():
    x = np.random.default_rng(3).standard_normal(1000).astype(np.float32)
    km = Q.QuantizedKmeans(8, init="cbrt")
    c, ct = km.compress(x), km.compress(torch.from_numpy(x))
    assert isinstance(ct.compressed_data, torch.Tensor) and ct.compressed_data.dtype == torch.int8
    assert np.array_equal(ct.compressed_data.numpy(), c.compressed_data) and np.array_equal(ct.q, c.q)
    dec = km.decompress(ct)
    assert isinstance(dec, torch.Tensor) and np.array_equal(dec.numpy(), km.decompress(c))
    assert km.iscompressed(c) and km.iscompressed([c, x]) == [True, False]
    both = km.compress([x, x[:500]])
    assert [b.n_iter > 0 for b in both] == [True, True] and km.decompress(both)[1].shape == (500,)


# ---------------------------------------------------------------------------
# decisive elements (kmeans_cases.py states each case's arithmetic)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(kc.SMALL))
def test_decisive_elements(name):
    """Each case against the oracle, its stated outcome, and (where it is aimed
    at one) the wrong implementation it catches: that variant of the oracle
    gives the probe another label.  boundary: ``<`` against ``<=``; half_up:
    round-half-down; sum32: a 32-bit sum; empty_cluster and three_steps: the
    kept centre and the step count."""
    case = kc.SMALL[name]()
    c = _against_oracle(case["x"], 8, case["K"], case["init"], case["max_iter"])
    assert c.n_iter == case["n_iter"]
    assert int(c.compressed_data[case["probe"]]) + 128 == case["label"]
    if case["catches"]:
        wrong = _oracle(case["x"], case["K"], case["init"], case["max_iter"], case["catches"])[0]
        assert wrong[case["probe"]] != case["label"], case["catches"]
    if name == "boundary":
        assert int(c.compressed_data[list(case["x"]).index(201.0)]) + 128 == 1  # b_0 + 1 goes up
    if name == "empty_cluster":
        assert c.q[1, 0] == float(1 << 31) and 1 not in set(c.compressed_data.astype(int) + 128)


@pytest.mark.parametrize("name", sorted(kc.POSITIONED))
def test_decisive_elements_among_fillers(name):
    """What test_gpu_kmeans.py places at every kind of position: the outcome does not depend on it."""
    for pos in (0, 255, -1):
        case = kc.POSITIONED[name](300, pos)
        c = _against_oracle(case["x"], 8, case["K"], case["init"], case["max_iter"])
        assert c.n_iter == case["n_iter"] and int(c.compressed_data[case["probe"]]) + 128 == case["label"]


def test_a_sum_beyond_2_to_the_53_is_exact():
    """Float sums.  An image is below 2^32 and a tensor has fewer than 2^32
    elements, so a cluster's sum stays below 2^64 and passes 2^53 from 2^21
    elements on: sum53 has 2^21 + 69.  The numpy form gives the stated
    outcome; one step of the oracle agrees, and the oracle adding in float64
    loses the half that decides the rounding and moves the probe."""
    case = kc.sum53()
    c = Q.QuantizedKmeans(8, 2, init=case["init"], max_iter=1).compress(case["x"])
    assert c.n_iter == 1 and int(c.compressed_data[case["probe"]]) + 128 == case["label"]
    us = [int(v) for v in case["x"]]  # s = 1: the image is the data
    c0 = [int(v) for v in case["init"]]
    exact, floating = o.step(us, c0), o.step(us, c0, "float_sums")
    V = kc.U - 3
    assert sum(us[3:]) > 1 << 53 and exact == [(1 << 30) + 1, V + 1] and floating == [(1 << 30) + 1, V]
    assert np.array_equal(_bits(c.q.reshape(-1)), _bits(np.array([float(v) for v in exact])))
    probe = [us[case["probe"]]]
    assert o.labels(probe, exact) == [0] and o.labels(probe, floating) == [1]
    labels = c.compressed_data.astype(np.int64) + 128
    assert np.array_equal(labels, np.array([0, 0, 0] + [1] * (len(us) - 3)))


def test_max_iter_bounds_the_steps():
    x = kc.data("normal", np.float32)
    c = Q.QuantizedKmeans(8, init="cbrt", max_iter=5).compress(x)
    assert c.n_iter == 5


# ---------------------------------------------------------------------------
# refusals and edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_refusals(dt):
    km = Q.QuantizedKmeans(8, init="cbrt")
    x = np.random.default_rng(0).standard_normal(100).astype(dt)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[50] = bad
        with pytest.raises(ValueError, match=r"^quantized entry \[0\]: "):
            km.compress(y)
    with pytest.raises(ValueError, match=r"^quantized entry \[0\]: .*constant tensor"):
        km.compress(np.full(100, 1.5, dtype=dt))
    with pytest.raises(ValueError, match=r"^quantized entry \[0\]: "):
        km.compress(np.zeros(0, dtype=dt))
    with pytest.raises(ValueError, match=r"^quantized entry \[1\]: "):
        km.compress([x, np.full(100, 1.5, dtype=dt)])
    if dt == np.float64:  # a range too small for s = U / (mx - mn) to be finite
        with pytest.raises(ValueError, match=r"^quantized entry \[0\]: .*too small"):
            km.compress(np.array([0.0] * 50 + [5e-324] * 50))
    for ints in (np.arange(100), np.arange(100, dtype=np.int8), np.arange(4)):
        with pytest.raises(TypeError, match="float32 or float64"):
            km.compress(ints)


def test_too_few_elements_pass_through():
    km = Q.QuantizedKmeans(8, init="cbrt")
    for n in (1, 7, 8):
        x = np.arange(n, dtype=np.float32)
        c = km.compress(x)
        assert c.compressed_data is x and c.q is None and c.origin_type is None and c.quant_bits == 8
        assert km.decompress(c) is x
    assert km.compress(np.arange(9, dtype=np.float32)).q.shape == (8, 1)


def test_the_constructor_refuses():
    for kw in (dict(n_clusters=1), dict(n_clusters=0), dict(quant_bits=4, n_clusters=17), dict(n_clusters=257)):
        with pytest.raises(ValueError, match="n_clusters must be in 2"):
            Q.QuantizedKmeans(**{"quant_bits": 8, "init": "cbrt", **kw})
    with pytest.raises(ValueError, match="init=None"):
        Q.QuantizedKmeans(8)
    with pytest.raises(ValueError, match="init=None"):
        Q.QuantizedKmeans(8, 8, None)
    with pytest.raises(ValueError, match="'cbrt' or an array"):
        Q.QuantizedKmeans(8, init="k-means++")
    for init in (np.array([2.0, 1.0]), np.array([1.0, 2.0, 3.0]), np.array([1, 2]), np.array([np.nan, 1.0])):
        with pytest.raises(ValueError, match="non-decreasing"):
            Q.QuantizedKmeans(8, 2, init=init)
    with pytest.raises(ValueError, match="max_iter"):
        Q.QuantizedKmeans(8, init="cbrt", max_iter=0)
    with pytest.raises(RuntimeError, match="between 0 and 64"):
        Q.QuantizedKmeans(0, 2, init="cbrt")
    assert Q.QuantizedKmeans(8, init="cbrt").n_clusters == 8  # the reference's default: quant_bits
    assert Q.QuantizedKmeans(16, 300, init="cbrt").np_type == np.int16


def test_the_factory_builds_it_with_an_init_only():
    km = C.get("quantized_kmeans", dict(quant_bits=8, n_clusters=16, init="cbrt", max_iter=9))
    assert isinstance(km, C.QuantizedKmeans) and (km.n_clusters, km.max_iter) == (16, 9)
    for params in ({}, None, dict(quant_bits=8), dict(init=None)):
        with pytest.raises(ValueError, match=r"^Compressor 'quantized_kmeans' is not built: scikit-learn's randomly "
                                             r"initialised k-means has no definition to pin; pass init='cbrt'$"):
            C.get("quantized_kmeans", params)
    assert C.KmeansCompressData is Q.KmeansCompressData is Q.QuantizedKmeans.KmeansCompressData


def test_a_start_outside_the_range_is_clipped():
    x = np.random.default_rng(8).standard_normal(500)
    init = np.array([-100.0, 0.0, 100.0])
    c = _against_oracle(x, 8, 3, init)
    assert c.n_iter >= 2


def test_mixed_compressor_round_trip():
    x = np.random.default_rng(4).standard_normal((60, 50)).astype(np.float32)
    mixed = C.MixedCompressor(C.TopkSparse(0.8), C.QuantizedKmeans(8, 32, init="cbrt"))
    m = mixed.compress(x)
    assert isinstance(m, C.MixedCompressedData) and m.compressed_data.dtype == np.int8
    assert isinstance(m.compressed_participants[1], C.KmeansCompressData)
    dec = mixed.decompress(m)
    # the two compressors one after the other give the same
    sparse, km = C.TopkSparse(0.8), C.QuantizedKmeans(8, 32, init="cbrt")
    s = sparse.compress(x)
    assert s.compressed_data.size == 600
    s.compressed_data = km.decompress(km.compress(s.compressed_data))
    assert len(np.unique(s.compressed_data)) <= 32
    assert dec.shape == x.shape and np.array_equal(dec, sparse.decompress(s))
    swapped = C.get("mixed_compressor", [dict(name="quantized_kmeans", params=dict(init="cbrt")),
                                         dict(name="topk_sparse", params=dict(sparse_rate=0.8))])
    assert isinstance(swapped.comressors[1], C.QuantizedKmeans)


@pytest.mark.parametrize("store", (np.int8, np.int16), ids=("i8", "i16"))
def test_a_code_outside_the_clusters_raises_and_names_its_position(store):
    bits = 8 if store == np.int8 else 16
    half, K = 1 << (bits - 1), 20
    q = np.arange(K, dtype=np.float64).reshape(-1, 1)
    codes = (np.arange(1000) % K - half).astype(store)
    km = Q.QuantizedKmeans(bits, K, init="cbrt")
    assert np.array_equal(km.decompress(Q.KmeansCompressData(codes, bits, np.dtype(np.float64), q)),
                          (np.arange(1000) % K).astype(np.float64))
    for where in ((0,), (999,), (500, 300, 999)):
        wrong = codes.copy()
        wrong[list(where)] = K - half
        with pytest.raises(ValueError, match=rf"outside the {K} clusters at position {min(where)}$"):
            km.decompress(Q.KmeansCompressData(wrong, bits, np.dtype(np.float64), q))
    with pytest.raises(ValueError, match="codes"):  # the storage type follows quant_bits
        km.decompress(Q.KmeansCompressData(codes.astype(np.int32), bits, np.dtype(np.float64), q))
    low = np.array([-9, -8], dtype=np.int8)  # at 4 bits the code -9 is the label -1
    with pytest.raises(ValueError, match="at position 0$"):
        Q.QuantizedKmeans(4, 10, init="cbrt").decompress(
            Q.KmeansCompressData(low, 4, np.dtype(np.float32), np.arange(10, dtype=np.float32).reshape(-1, 1)))
