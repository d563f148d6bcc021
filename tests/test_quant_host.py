"""The quantized compressors on the host (sfl_amd/utils/quantized.py, the
numpy form): bit for bit against what the reference's own classes gave
(tests/golden/quant_reference.npz, made by tests/golden/make_quant_golden.py),
the reference's own round-trip contract, and every refusal."""
import numpy as np
import pytest

import quant_cases as qc
from sfl_amd.utils import compressor as cmod
from sfl_amd.utils import quantized as Q

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def golden():
    return qc.Golden()


def make(scheme):
    cls, kw = qc.SCHEMES[scheme]
    return getattr(Q, cls)(**kw)


def check_against(golden, k, scheme, x):
    comp = make(scheme)
    c = comp.compress(x)
    want = golden.codes(k)
    assert c.compressed_data.dtype == want.dtype and c.compressed_data.shape == want.shape, k
    assert np.array_equal(c.compressed_data, want), k
    p0, p1 = qc.params_of(scheme, c)
    assert (p0, p1) == golden.params(k), k  # by value: a zero's sign is free
    dec = comp.decompress(c)
    assert dec.dtype == x.dtype and dec.shape == x.shape, k
    assert np.array_equal(qc.digest(dec), golden.dec(k)), k


@pytest.mark.parametrize("scheme", list(qc.SCHEMES))
def test_the_numpy_form_is_the_reference_bit_for_bit(golden, scheme):
    cases = [c for c in qc.all_cases() if c[1] == scheme]
    assert len(cases) == len(qc.DTYPES) * len(qc.N) * len(qc.SCALES)
    for k, _, dt, n, si in cases:
        check_against(golden, k, scheme, qc.case_input(golden.seed(k), n, qc.SCALES[si], dt))


@pytest.mark.parametrize("scheme", qc.TIE_SCHEMES)
@pytest.mark.parametrize("dt", qc.DTYPES)
def test_rounding_ties_go_to_even_as_in_the_reference(golden, scheme, dt):
    x = qc.tie_input(scheme, dt)
    check_against(golden, qc.tie_key(scheme, dt), scheme, x)
    c = make(scheme).compress(x)
    if scheme == "zp8":
        assert c.scale == 2.0 ** -8 and c.nudged_zero_point == 0
        k = np.arange(-128, 127)
        even = np.where(k % 2 == 0, k, k + 1)  # k + 0.5 to the even neighbour
        assert np.array_equal(c.compressed_data, np.concatenate([[-128, 127], even]))
    else:
        assert c.scale == 1.0
        assert int(c.compressed_data.max()) == {"e4m3": 126, "e5m2": 123}[scheme]
        assert not np.any(c.compressed_data[1:] % 2)  # qm even, mant_len even: every tie's code is even


# the reference's own contract, tests/utils/test_compressor.py:34-41
@pytest.mark.parametrize("shape", [(10, 10), (10, 10, 10, 10)])
@pytest.mark.parametrize("scheme,atol", [("zp8", 0.2), ("lstm8", 0.2), ("e4m3", 0.2)])
def test_the_references_round_trip_contract(scheme, shape, atol):
    data = np.random.default_rng(20).uniform(low=-5, high=5, size=shape)
    comp = make(scheme)
    c = comp.compress(data)
    assert isinstance(c, Q.QuantizedCompressedData) and isinstance(c, cmod.QuantizedCompressedData)
    plain = comp.decompress(c)
    err = float(np.max(np.abs(data - plain)))
    print(f"{scheme} {shape}: max error {err:.3f}")
    np.testing.assert_allclose(data, plain, atol=atol)


@pytest.mark.parametrize("shape", [(10, 10), (10, 10, 10, 10)])
def test_e5m2_round_trip_within_a_quarter_of_a_binade(shape):
    """E5M2 has two mantissa bits: codes are 1/4 of a binade apart relative
    to its lower end, so the error is at most 1/8 of the binade's lower end,
    which is below max|x| / 8 (the scale puts max|x| at 0.875 of a binade's top)."""
    data = np.random.default_rng(21).uniform(low=-5, high=5, size=shape)
    comp = make("e5m2")
    plain = comp.decompress(comp.compress(data))
    err = float(np.max(np.abs(data - plain)))
    print(f"e5m2 {shape}: max error {err:.3f}")
    assert err <= float(np.max(np.abs(data))) / 8


def test_lists_single_arrays_and_iscompressed():
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((4, 5)).astype(np.float32), rng.standard_normal(7)
    for scheme in qc.SCHEMES:
        comp = make(scheme)
        one = comp.compress(a)
        assert isinstance(one, Q.QuantizedCompressedData) and comp.iscompressed(one) is True
        assert one.compressed_data.shape == a.shape and one.origin_type == np.float32
        many = comp.compress([a, b])
        assert isinstance(many, list) and comp.iscompressed(many) == [True, True]
        assert comp.iscompressed([a, many[1]]) == [False, True] and comp.iscompressed(a) is False
        assert isinstance(comp.compress((a, b)), list)
        back = comp.decompress(many)
        assert isinstance(back, list) and [x.dtype for x in back] == [np.float32, np.float64]
        assert np.array_equal(back[0], comp.decompress(one))
        for bad in (None, 3.0, {"a": a}):
            with pytest.raises(TypeError, match="invalid data"):
                comp.compress(bad)
    z = make("zp8").compress(a)
    assert (z.quant_bits, type(z.nudged_zero_point)) == (8, int) and type(z.scale) is np.float32
    s = make("lstm16").compress(b)
    assert s.compressed_data.dtype == np.int16 and type(s.rqm) is int and type(s.q) is np.float64
    assert make("zp4").compress(a).compressed_data.dtype == np.int8
    assert type(make("e5m2").compress(a).scale) is np.float32


def test_cpu_tensors_run_numpy_and_stay_tensors():
    a = np.random.default_rng(4).standard_normal((3, 9)).astype(np.float32)
    for scheme in qc.SCHEMES:
        comp = make(scheme)
        c, ct = comp.compress(a), comp.compress(torch.from_numpy(a))
        assert isinstance(ct.compressed_data, torch.Tensor) and not ct.is_device
        assert np.array_equal(ct.compressed_data.numpy(), c.compressed_data)
        dt = comp.decompress(ct)
        assert isinstance(dt, torch.Tensor) and np.array_equal(dt.numpy(), comp.decompress(c))


BAD_RANGE = {
    "a NaN": np.array([1.0, np.nan, 3.0]),
    "a NaN first": np.array([np.nan, 1.0, 3.0]),
    "an inf": np.array([1.0, np.inf, 3.0]),
    "a negative inf": np.array([-np.inf, 1.0]),
    "a constant": np.full(5, 2.5),
    "all zero": np.zeros(4),
    "one element": np.array([1.5]),
    "empty": np.zeros(0),
    "a range that overflows": np.array([-3e38, 3e38]),
}


@pytest.mark.parametrize("what", list(BAD_RANGE))
@pytest.mark.parametrize("scheme", ["zp8", "zp16", "lstm8", "lstm16"])
def test_zero_point_and_lstm_refuse_a_range_that_is_not_finite_and_positive(scheme, what):
    x = BAD_RANGE[what].astype(np.float32)
    comp = make(scheme)
    with pytest.raises(ValueError, match=r"quantized entry \[0\].*not finite and positive"):
        comp.compress(x)
    good = np.array([0.0, 1.0], dtype=np.float32)
    with pytest.raises(ValueError, match=r"quantized entry \[2\]"):
        comp.compress([good, good, x])


def test_lstm_refuses_a_range_too_small_to_divide_by():
    tiny = np.array([0.0, 1e-45], dtype=np.float32)  # 255 / 1e-45 overflows
    with pytest.raises(ValueError, match=r"quantized entry \[0\].*too small"):
        make("lstm8").compress(tiny)
    assert make("zp8").compress(tiny * 255).compressed_data.tolist() == [-128, 127]  # zero-point handles denormals


@pytest.mark.parametrize("scheme", ["e4m3", "e5m2"])
def test_fp8_refuses_nan_and_inf_and_takes_zeros(scheme):
    comp = make(scheme)
    for bad in (np.array([1.0, np.nan]), np.array([np.inf, 1.0]), np.array([-np.inf, 1.0])):
        with pytest.raises(ValueError, match=r"quantized entry \[1\].*largest magnitude"):
            comp.compress([np.ones(2, dtype=np.float32), bad.astype(np.float32)])
    with pytest.raises(ValueError, match="too small to scale"):
        comp.compress(np.array([0.0, 1e-45], dtype=np.float32))
    z = comp.compress(np.zeros((2, 3), dtype=np.float32))
    assert z.scale == qc.FP8[scheme][0] and not z.compressed_data.any()
    assert np.array_equal(comp.decompress(z), np.zeros((2, 3), dtype=np.float32))
    e = comp.compress(np.zeros(0))
    assert e.compressed_data.shape == (0,) and comp.decompress(e).shape == (0,)
    # constants and single elements are fine too
    assert comp.compress(np.array([-2.0])).compressed_data.tolist() == [-{"e4m3": 126, "e5m2": 123}[scheme]]


def test_fp8_decodes_minus_128_as_128():
    for scheme, (mx, ml, off) in qc.FP8.items():
        comp = make(scheme)
        c = Q.FPCompressData(np.array([-128, 127, 0, 1, -1], dtype=np.int8), 8, np.float32, np.float32(2.0))
        dec = comp.decompress(c)
        assert dec.dtype == np.float32
        assert dec[0] == -np.ldexp(0.5, 128 // ml - off) / 2.0
        assert dec[2] == 0 and dec[3] == -dec[4] == np.ldexp((1 / ml + 1) / 2, -off) / 2.0


def test_tiny_fp8_values_keep_the_references_floor():
    """A scaled magnitude below 2^-exp_offset keeps its mantissa field only:
    it decodes into [2^-(exp_offset+1), 2^-exp_offset) / scale whatever its
    exponent was, or to 0 when the mantissa field is 0."""
    x = np.array([448.0, 1.5e-6, -1.5e-6, 0.0, 1e-6], dtype=np.float32)  # 1.5e-6 = 0.786 * 2^-19, 1e-6 = 0.524 * 2^-19
    comp = make("e4m3")
    c = comp.compress(x)
    assert c.scale == 1 and c.compressed_data.tolist() == [126, 5, -5, 0, 0]
    dec = comp.decompress(c)
    assert dec.tolist() == [448.0, 0.8125 * 2.0 ** -6, -0.8125 * 2.0 ** -6, 0.0, 0.0]


@pytest.mark.parametrize("dt", qc.DTYPES)
@pytest.mark.parametrize("bits", [8, 16])
def test_lstm_codes_saturate_where_the_reference_wraps(bits, dt):
    """[0.5, 3, 2^bits - 0.5]: q = 1 exactly and q min = 0.5 rounds to 0, so
    rqm = 2^(bits-1), the minimum codes to -2^(bits-1) (it always does) and
    the maximum to rint(2^bits - 0.5) - 2^(bits-1) = +2^(bits-1), one past the
    storage range.  The reference's cast wraps it to the minimum's code; here
    it saturates, and the largest element decodes as the largest."""
    x = qc.lstm_saturating(bits, dt)
    half = 1 << (bits - 1)
    comp = make(f"lstm{bits}")
    c = comp.compress(x)
    assert (c.q, c.rqm) == (1.0, half) and type(c.q) is dt
    assert (np.rint(c.q * x) - dt(c.rqm)).tolist() == [-half, 3 - half, half]  # before the clamp
    assert c.compressed_data.dtype == comp.np_type
    assert c.compressed_data.tolist() == [-half, 3 - half, half - 1]
    dec = comp.decompress(c)
    assert dec.dtype == dt and dec.tolist() == [0.0, 3.0, 2.0 * half - 1]


def test_integer_data_and_bad_widths():
    for scheme in qc.SCHEMES:
        for bad in (np.arange(6), np.arange(6, dtype=np.int64).reshape(2, 3), np.ones(3, dtype=bool),
                    np.ones(3, dtype=np.float16)):
            with pytest.raises(TypeError, match="float32 or float64"):
                make(scheme).compress(bad)
        with pytest.raises(TypeError):
            make(scheme).compress(torch.arange(6))
    with pytest.raises(TypeError, match="floating-point"):
        Q.QuantizedFP(16).compress(np.arange(6))
    for cls in (Q.QuantizedZeroPoint, Q.QuantizedLSTM, Q.QuantizedFP):
        for bits in (0, -1, 65):
            with pytest.raises(RuntimeError, match="between 0 and 64"):
                cls(bits)
    with pytest.raises(RuntimeError, match="8/16/32/64"):
        Q.QuantizedFP(12)
    with pytest.raises(RuntimeError, match="E4M3/E5M2"):
        Q.QuantizedFP(8, format="E3M4")
    assert Q.QuantizedZeroPoint(3).np_type is np.int8 and Q.QuantizedLSTM(9).np_type is np.int16
    assert Q.QuantizedZeroPoint(17).np_type is np.int32 and Q.QuantizedLSTM(64).np_type is np.int64


def test_wide_codes_on_the_host():
    x = np.random.default_rng(5).standard_normal(100)
    for cls in (Q.QuantizedZeroPoint, Q.QuantizedLSTM):
        comp = cls(24)
        c = comp.compress(x)
        assert c.compressed_data.dtype == np.int32
        np.testing.assert_allclose(comp.decompress(c), x, atol=1e-6)
    c = Q.QuantizedLSTM(32).compress(x.astype(np.float32))  # float32(2^31 - 1) is 2^31: the clamp stays inside
    assert c.compressed_data.dtype == np.int32 and c.compressed_data.max() < 2 ** 31 - 1


def test_decompress_refuses_codes_of_the_wrong_width():
    c = make("zp8").compress(np.arange(4, dtype=np.float32))
    c.compressed_data = c.compressed_data.astype(np.int16)
    with pytest.raises(ValueError, match="int16 codes"):
        make("zp8").decompress(c)


def test_fp_casts():
    x = np.random.default_rng(6).standard_normal((5, 3))
    for bits, dt in ((16, np.float16), (32, np.float32), (64, np.float64)):
        comp = Q.QuantizedFP(bits)
        c = comp.compress(x)
        assert c.compressed_data.dtype == dt and c.scale is None and c.origin_type == np.float64
        assert np.array_equal(c.compressed_data, x.astype(dt))
        back = comp.decompress(c)
        assert back.dtype == np.float64 and np.array_equal(back, x.astype(dt).astype(np.float64))
        assert c.nbytes == x.size * bits // 8
        t = comp.compress(torch.from_numpy(x))
        assert isinstance(t.compressed_data, torch.Tensor) and t.compressed_data.dtype == getattr(torch, f"float{bits}")
        assert comp.decompress(t).dtype == torch.float64


def test_to_cpu_and_nbytes():
    a = np.random.default_rng(7).standard_normal((6, 7)).astype(np.float32)
    for scheme, per in (("zp8", 1), ("zp16", 2), ("zp4", 1), ("lstm8", 1), ("lstm16", 2), ("e4m3", 1), ("e5m2", 1)):
        comp = make(scheme)
        c = comp.compress(a)
        assert c.nbytes == a.size * per and not c.is_device
        assert cmod.payload_nbytes(c) == c.nbytes
        assert cmod.payload_nbytes([c, a, None]) == c.nbytes + a.nbytes
        h = c.to("cpu")
        assert type(h) is type(c) and isinstance(h.compressed_data, np.ndarray)
        assert np.array_equal(h.compressed_data, c.compressed_data)
        assert qc.params_of(scheme, h) == qc.params_of(scheme, c) and h.origin_type == c.origin_type
        assert np.array_equal(comp.decompress(h), comp.decompress(c))
        t = comp.compress(torch.from_numpy(a)).to("cpu")  # CPU-tensor codes come back as numpy
        assert isinstance(t.compressed_data, np.ndarray) and np.array_equal(t.compressed_data, c.compressed_data)


def test_the_names_are_re_exported():
    for name in ("QuantizedZeroPoint", "QuantizedLSTM", "QuantizedFP", "QuantizedCompressedData"):
        assert getattr(cmod, name) is getattr(Q, name)
