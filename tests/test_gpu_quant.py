"""The sa_quant kernels on the GPU against the numpy form
(sfl_amd/utils/quantized.py on host arrays, itself pinned to the reference by
tests/test_quant_host.py), bit for bit: the range, the code kernels, the
decoders over every code, and the classes on device tensors.  Every kernel
output is a view into a larger allocation whose 64 guard elements on both
sides must come back unchanged."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import quant_cases as qc  # noqa: E402
from gpu_copies import DEV, _bits, _dev, _host  # noqa: E402

from sfl_amd.utils import quantized as Q  # noqa: E402

pytestmark = pytest.mark.gpu
# below 16: the scalar head and tail alone; 1023 / 1025: around one block's 256
# decoder runs of 4; 65,537: several blocks and a one-element tail; 2^20 + 3:
# 256 blocks.  WRAP is past the largest grid (the fp8 decoder's 1024 blocks of
# 256 threads with 16 elements each; 512 blocks elsewhere), so every kernel's
# grid-stride loop comes round again.
N = (2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 65537, 2**20 + 3)
WRAP = 1024 * 256 * 16 + 4099
DTYPES = (np.float32, np.float64)
IDS = ["f32", "f64"]
GUARD = 64
PAT_F, PAT_Q = 12345.0, 0x5A


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _devt(a):
    """A host array on the device in its own shape, through pinned memory."""
    from sfl_amd import hostpipe as H

    return H.h2d(a, torch.device(DEV))


def _tdt(dt):
    return Q._torch_dtype(np.dtype(dt))


def make(scheme):
    cls, kw = qc.SCHEMES[scheme]
    return getattr(Q, cls)(**kw)


def _guarded(n, tdt, fill, odd=False):
    """(the whole allocation, the view of n elements inside it, its offset);
    ``odd``: the view starts one element further, so it is element-aligned only."""
    lo = GUARD + (1 if odd else 0)
    big = torch.full((lo + n + GUARD,), fill, dtype=tdt, device=DEV)
    return big, big[lo:lo + n], lo


def _guards_intact(big, lo, n, fill):
    h = _host(big)
    return bool(np.all(h[:lo] == fill) and np.all(h[lo + n:] == fill))


def _same(a, b):
    """Equal by value, NaN equal to NaN (the sign of a zero is free)."""
    return bool(a == b or (np.isnan(a) and np.isnan(b)))


def _range(xd):
    """(min, max, max|x|) by the kernel, into guarded words."""
    from sfl_amd import kernels as K

    big, out3, lo = _guarded(3, xd.dtype, PAT_F)
    scratch = torch.empty(K.quant_scratch_bytes(xd.numel(), xd.dtype), dtype=torch.uint8, device=DEV)
    K.quant_range(xd, scratch, out3)
    w = _host(out3)
    assert _guards_intact(big, lo, 3, PAT_F)
    return w


def _data(dt, n, s=1.0):
    return (np.random.default_rng(7 * n + 1).standard_normal(n) * s).astype(dt)


# ---------------------------------------------------------------------------
# the range
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_range_finds_an_extreme_wherever_it_sits(dt):
    """The extreme at index 0, at n - 1, and on both sides of every boundary
    of the kernel's lane map: a wave's and a block's 16-byte vectors (64, 256
    vectors of 4 or 2 elements), the four vectors a thread takes per
    iteration, and the scalar head and tail of an element-aligned view."""
    per = 16 // np.dtype(dt).itemsize
    for n in N:
        x = np.clip(_data(dt, n), -4, 4)
        part = np.sort(x)
        lo2, hi2 = part[:2], part[-2:]  # the two least and the two largest: what is left without x[p]
        edges = {0, n - 1, n // 2}
        for b in (64 * per, 256 * per, 1024 * per, 4096 * per, 1024 * 256 * per):
            edges |= {b - 1, b, b + 1}
        for mis in (False, True):
            xd = _dev(x, misalign=mis)
            w = _range(xd)
            assert (w[0], w[1], w[2]) == (x.min(), x.max(), np.abs(x).max()), (n, mis)
            for p in sorted(e for e in edges if 0 <= e < n):
                for v in (-11.0, 11.0):
                    xd[p] = v
                    w = _range(xd)
                    want = (min(v, lo2[1] if x[p] == lo2[0] else lo2[0]), max(v, hi2[0] if x[p] == hi2[1] else hi2[1]),
                            11.0)
                    assert (w[0], w[1], w[2]) == want, (n, mis, p, v)
                xd[p] = float(x[p])


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_range_propagates_nan_and_keeps_zeros_and_denormals(dt):
    tiny = np.nextafter(dt(0), dt(1))
    for n in (2, 5, 257, 1025, 65537):
        x = np.resize(np.array([0.0, -0.0, tiny, -tiny, 3 * tiny, -0.0], dtype=dt), n)
        for mis in (False, True):
            w = _range(_dev(x, misalign=mis))
            assert all(_same(a, b) for a, b in zip(w, (x.min(), x.max(), np.abs(x).max()))), (n, mis, w)
            assert n < 3 or (w[0], w[1], w[2]) == (-tiny, 3 * tiny if n > 4 else tiny, 3 * tiny if n > 4 else tiny)
        y = _data(dt, n)
        for p in sorted({0, n // 2, n - 1}):
            z = y.copy()
            z[p] = np.nan
            w = _range(_dev(z, misalign=bool(p & 1)))
            assert np.isnan(w).all(), (n, p, w)
    z = np.zeros(300, dtype=dt)
    z[7] = -np.inf
    w = _range(_dev(z))
    assert w[0] == -np.inf and w[1] == 0 and w[2] == np.inf
    w = _range(torch.empty(0, dtype=_tdt(dt), device=DEV))
    assert w[0] == np.inf and w[1] == -np.inf and w[2] == 0


# ---------------------------------------------------------------------------
# the code kernels
# ---------------------------------------------------------------------------
def _encode(scheme, c, xd, mis):
    """The codes of the device vector ``xd`` by the kernel, with the host
    object ``c``'s scalars, into a guarded (and maybe odd) view."""
    from sfl_amd import _lib as L
    from sfl_amd import kernels as K

    n, store = xd.numel(), c.compressed_data.dtype
    big, q, lo = _guarded(n, _tdt(store), PAT_Q, odd=mis)
    T = c.origin_type.type
    if scheme.startswith("zp"):
        b = c.quant_bits
        K.quant_affine(xd, L.SA_QUANT_ZERO_POINT, float(c.scale), float(c.nudged_zero_point), -(1 << (b - 1)),
                       (1 << (b - 1)) - 1, q)
    elif scheme.startswith("lstm"):
        info = np.iinfo(store)
        K.quant_affine(xd, L.SA_QUANT_LSTM, float(c.q), float(T(c.rqm)), int(info.min), int(info.max), q)
    else:
        _, ml, off = qc.FP8[scheme]
        K.quant_fp8(xd, float(c.scale), ml, off, q)
    got = _host(q)
    assert _guards_intact(big, lo, n, PAT_Q), (scheme, n, mis)
    return got


def _decode(scheme, c, qd, mis):
    from sfl_amd import _lib as L
    from sfl_amd import kernels as K

    n, T = qd.numel(), c.origin_type.type
    big, out, lo = _guarded(n, _tdt(c.origin_type), PAT_F, odd=mis)
    if scheme.startswith("zp"):
        K.dequant_affine(qd, L.SA_QUANT_ZERO_POINT, float(c.scale), float(c.nudged_zero_point), out)
    elif scheme.startswith("lstm"):
        K.dequant_affine(qd, L.SA_QUANT_LSTM, float(c.q), float(T(c.rqm)), out)
    else:
        _, ml, off = qc.FP8[scheme]
        K.dequant_fp8(qd, float(c.scale), ml, off, out)
    got = _host(out)
    assert _guards_intact(big, lo, n, PAT_F), (scheme, n, mis)
    return got


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_codes_and_round_trips_match_the_numpy_form(dt):
    """Every scheme at every size, aligned and offset by one element on both
    sides; the two random families, both of them from 65,537 on."""
    for i, n in enumerate(N):
        for si in ((0, 1) if n >= 65537 else (i % 2,)):
            x = qc.case_input(1000 + n, n, qc.SCALES[si], dt)
            xds = {mis: _dev(x, misalign=mis) for mis in (False, True)}
            for scheme in qc.SCHEMES:
                comp = make(scheme)
                c = comp.compress(x)
                dec = comp.decompress(c)
                for mis in (False, True):
                    got = _encode(scheme, c, xds[mis], mis)
                    assert got.dtype == c.compressed_data.dtype
                    assert np.array_equal(got, c.compressed_data), (scheme, n, si, mis)
                    back = _decode(scheme, c, _dev(c.compressed_data, misalign=mis), mis)
                    assert np.array_equal(_bits(back), _bits(dec)), (scheme, n, si, mis)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_the_grid_stride_loops_come_round(dt):
    """One size past the grid's bound: the range and, for one scheme of each
    kernel and both code widths, the codes and the round trip."""
    x = qc.case_input(77, WRAP, 5, dt)
    x[WRAP - 3], x[WRAP // 2 + 1] = -400, 300  # the extremes behind the first round of the grid
    xd = _dev(x)
    w = _range(xd)
    assert (w[0], w[1], w[2]) == (-400, 300, 400)
    for scheme in ("zp8", "lstm16", "e4m3"):
        comp = make(scheme)
        c = comp.compress(x)
        assert np.array_equal(_encode(scheme, c, xd, False), c.compressed_data), scheme
        back = _decode(scheme, c, _dev(c.compressed_data), False)
        assert np.array_equal(_bits(back), _bits(comp.decompress(c))), scheme


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("bits", [8, 16])
def test_lstm_codes_saturate_on_the_device(bits, dt):
    """The input whose largest element codes to +2^(bits-1) before the clamp
    (tests/quant_cases.py): 2^(bits-1) - 1 from the kernel, in the scalar head
    and tail (n = 3) and in the packed main body (n = 1025), never the
    wrapped -2^(bits-1); the class on the device gives the host's bits."""
    half = 1 << (bits - 1)
    comp = make(f"lstm{bits}")
    for n in (3, 1025):
        x = qc.lstm_saturating(bits, dt, n)
        want = np.resize(np.array([-half, 3 - half, half - 1]), n)
        c = comp.compress(x)
        assert (c.q, c.rqm) == (1.0, half) and c.compressed_data.tolist() == want.tolist()
        for mis in (False, True):
            got = _encode(f"lstm{bits}", c, _dev(x, misalign=mis), mis)
            assert got.tolist() == want.tolist(), (n, mis)
        d = comp.compress(_devt(x))
        assert d.is_device and (d.q, d.rqm) == (c.q, c.rqm)
        assert _host(d.compressed_data).tolist() == want.tolist(), n
        dec = _host(comp.decompress(d))
        assert dec.dtype == dt and dec.tolist() == np.resize(np.array([0.0, 3.0, 2.0 * half - 1]), n).tolist()


def test_mixed_alignment_takes_the_element_path():
    """The codes offset by one element and the data aligned (and the other way
    round): the head that aligns the codes leaves the floats unaligned."""
    n = 1025
    for dt in DTYPES:
        x = qc.case_input(5, n, 5, dt)
        for scheme in ("zp8", "lstm16", "e4m3"):
            comp = make(scheme)
            c = comp.compress(x)
            for mis_x, mis_q in ((False, True), (True, False)):
                got = _encode(scheme, c, _dev(x, misalign=mis_x), mis_q)
                assert np.array_equal(got, c.compressed_data), (scheme, dt, mis_x, mis_q)
                back = _decode(scheme, c, _dev(c.compressed_data, misalign=mis_q), mis_x)
                assert np.array_equal(_bits(back), _bits(comp.decompress(c))), (scheme, dt, mis_x, mis_q)


@pytest.fixture(scope="module")
def golden():
    return qc.Golden()


def _check_device_case(golden, k, scheme, x):
    comp = make(scheme)
    c = comp.compress(_devt(x))
    assert c.is_device and c.compressed_data.shape == x.shape
    assert np.array_equal(_host(c.compressed_data), golden.codes(k)), k
    assert qc.params_of(scheme, c) == golden.params(k), k
    dec = comp.decompress(c)
    assert dec.is_cuda and dec.dtype == _tdt(x.dtype)
    assert np.array_equal(qc.digest(_host(dec)), golden.dec(k)), k


def test_the_fixtures_cases_on_the_device(golden):
    for k, scheme, dt, n, si in qc.all_cases():
        _check_device_case(golden, k, scheme, qc.case_input(golden.seed(k), n, qc.SCALES[si], dt))


def test_the_tie_sets_on_the_device(golden):
    for scheme in qc.TIE_SCHEMES:
        for dt in DTYPES:
            _check_device_case(golden, qc.tie_key(scheme, dt), scheme, qc.tie_input(scheme, dt))


def test_a_denormal_scale_divides_as_numpy_does():
    """Small multiples of the least float32 denormal: scale is a denormal and
    x / scale a division of denormals."""
    tiny = np.nextafter(np.float32(0), np.float32(1))
    rng = np.random.default_rng(11)
    for n in (5, 257, 4099):
        for scheme, top in (("zp8", 1000), ("zp4", 1000), ("zp16", 2**20)):  # scale about 8, 133 and 32 denormal steps
            x = (rng.integers(-top, top + 1, n).astype(np.float32) * tiny).astype(np.float32)
            x[0], x[-1] = -top * tiny, top * tiny
            comp = make(scheme)
            c = comp.compress(x)
            assert 0 < c.scale < np.finfo(np.float32).tiny
            d = comp.compress(_devt(x))
            assert (d.scale, d.nudged_zero_point) == (c.scale, c.nudged_zero_point)
            assert np.array_equal(_host(d.compressed_data), c.compressed_data), (scheme, n)
            assert np.array_equal(_bits(_host(comp.decompress(d))), _bits(comp.decompress(c))), (scheme, n)


# ---------------------------------------------------------------------------
# the decoders over every code
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_every_affine_code_decodes_as_in_numpy(dt):
    x = qc.case_input(3, 999, 5, dt) + dt(1.25)
    for scheme, store in (("zp8", np.int8), ("zp4", np.int8), ("zp16", np.int16), ("lstm8", np.int8),
                          ("lstm16", np.int16)):
        comp = make(scheme)
        c = comp.compress(x)
        info = np.iinfo(store)
        c.compressed_data = np.arange(info.min, info.max + 1, dtype=np.int64).astype(store)
        want = comp.decompress(c)
        for mis in (False, True):
            got = _decode(scheme, c, _dev(c.compressed_data, misalign=mis), mis)
            assert np.array_equal(_bits(got), _bits(want)), (scheme, mis)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_every_fp8_code_decodes_as_in_numpy(dt):
    codes = np.arange(-128, 128, dtype=np.int64).astype(np.int8)
    for scheme in ("e4m3", "e5m2"):
        comp = make(scheme)
        for scale in (1.0, 448 / 3.7, 57344 / 1e-3):
            c = Q.FPCompressData(codes, 8, dt, dt(scale))
            want = comp.decompress(c)
            assert want[0] < 0 and np.isfinite(want).all()  # -128 is 128, negative
            for mis in (False, True):
                got = _decode(scheme, c, _dev(codes, misalign=mis), mis)
                assert np.array_equal(_bits(got), _bits(want)), (scheme, scale, mis)


# ---------------------------------------------------------------------------
# the classes on device tensors
# ---------------------------------------------------------------------------
def test_device_tensors_give_device_codes_and_the_hosts_bits():
    rng = np.random.default_rng(9)
    a = rng.standard_normal((33, 7)).astype(np.float32)
    b = rng.standard_normal((5, 4, 3, 2)) * 5
    for scheme in qc.SCHEMES:
        comp = make(scheme)
        host = comp.compress([a, b])
        mixed = comp.compress([_devt(a), b, _devt(b), torch.from_numpy(a)])
        assert [m.is_device for m in mixed] == [True, False, True, False]
        assert isinstance(mixed[3].compressed_data, torch.Tensor) and isinstance(mixed[1].compressed_data, np.ndarray)
        for m, h in zip(mixed, (host[0], host[1], host[1], host[0])):
            assert m.compressed_data.shape == h.compressed_data.shape and m.nbytes == h.nbytes
            assert Q._np_dtype(m.compressed_data.dtype) == h.compressed_data.dtype
            assert qc.params_of(scheme, m) == qc.params_of(scheme, h) and m.origin_type == h.origin_type
            assert np.array_equal(Q._host(m.compressed_data), h.compressed_data)
        back, want = comp.decompress(mixed), comp.decompress(host)
        assert back[0].is_cuda and back[2].is_cuda and isinstance(back[1], np.ndarray) and not back[3].is_cuda
        for g, w in zip(back, (want[0], want[1], want[1], want[0])):
            assert tuple(g.shape) == w.shape
            assert np.array_equal(_bits(Q._host(g)), _bits(w)), scheme
        # .to() both ways: the host object on the device decodes there, and back
        up = host[0].to(DEV)
        assert up.is_device and type(up) is type(host[0]) and up.compressed_data.dtype == mixed[0].compressed_data.dtype
        assert np.array_equal(_bits(_host(comp.decompress(up))), _bits(want[0]))
        down = mixed[2].to("cpu")
        assert not down.is_device and isinstance(down.compressed_data, np.ndarray)
        assert np.array_equal(_bits(comp.decompress(down)), _bits(want[1]))


def test_fp_casts_on_the_device_are_torchs():
    x = _devt(np.random.default_rng(2).standard_normal((4, 5)))
    for bits in (16, 32, 64):
        comp = Q.QuantizedFP(bits)
        c = comp.compress(x)
        assert c.is_device and c.compressed_data.dtype == getattr(torch, f"float{bits}") and c.scale is None
        back = comp.decompress(c)
        assert back.is_cuda and back.dtype == torch.float64
        assert np.array_equal(_host(back), _host(x.to(getattr(torch, f"float{bits}")).to(torch.float64)))


def _message(fn):
    with pytest.raises(ValueError) as e:
        fn()
    return str(e.value)


def test_the_refusals_on_the_device_use_the_hosts_words():
    good = np.array([0.0, 1.0, 2.0], dtype=np.float32)
    n = 4099
    base = np.random.default_rng(1).standard_normal(n).astype(np.float32)
    bad = {"constant": np.full(70, 2.5, np.float32), "single": np.array([1.5], np.float32),
           "empty": np.zeros(0, np.float32), "inf": np.where(np.arange(n) == 77, np.inf, base).astype(np.float32),
           "overflow": np.array([-3e38, 3e38], np.float32)}
    for p in (0, n // 2, n - 1):  # a NaN at the first, a middle and the last index
        z = base.copy()
        z[p] = np.nan
        bad[f"nan{p}"] = z
    for scheme in ("zp8", "zp16", "lstm8", "lstm16"):
        comp = make(scheme)
        for name, x in bad.items():
            on_host = _message(lambda: comp.compress([good, x]))
            on_dev = _message(lambda: comp.compress([_devt(good), _devt(x)]))
            assert on_dev == on_host and "[1]" in on_dev and "not finite and positive" in on_dev, (scheme, name)
    for scheme in ("e4m3", "e5m2"):
        comp = make(scheme)
        for name in ("inf", "nan0", f"nan{n // 2}", f"nan{n - 1}"):
            on_host = _message(lambda: comp.compress([good, bad[name]]))
            on_dev = _message(lambda: comp.compress([_devt(good),
                                                     _devt(bad[name])]))
            assert on_dev == on_host and "largest magnitude" in on_dev, (scheme, name)
        z = comp.compress(torch.zeros(300, device=DEV))
        assert z.scale == qc.FP8[scheme][0] and not _host(z.compressed_data).any()
        assert not _host(comp.decompress(z)).any()
        e = comp.compress(torch.zeros(0, device=DEV))
        assert e.is_device and e.compressed_data.numel() == 0 and comp.decompress(e).numel() == 0
    x = _devt(base)
    for cls in (Q.QuantizedZeroPoint, Q.QuantizedLSTM):
        with pytest.raises(ValueError, match="host arrays take any width"):
            cls(17).compress(x)
        with pytest.raises(TypeError, match="float32 or float64"):
            cls().compress(torch.arange(8, device=DEV))
        with pytest.raises(TypeError, match="float32 or float64"):
            cls().compress(x.to(torch.float16))
    with pytest.raises(TypeError, match="float32 or float64"):
        Q.QuantizedFP().compress(torch.arange(8, device=DEV))


def test_the_wrappers_check_their_tensors():
    from sfl_amd import kernels as K

    x = torch.zeros(8, device=DEV)
    q8, q16 = torch.zeros(8, dtype=torch.int8, device=DEV), torch.zeros(8, dtype=torch.int16, device=DEV)
    with pytest.raises(TypeError):
        K.quant_fp8(x, 1.0, 8, 6, q16)
    with pytest.raises(TypeError):
        K.quant_affine(x, 0, 1.0, 0.0, -128, 127, torch.zeros(8, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="one length"):
        K.quant_affine(x, 0, 1.0, 0.0, -128, 127, q8[:7])
    with pytest.raises(ValueError, match="contiguous"):
        K.dequant_affine(q16[::2], 0, 1.0, 0.0, x[:4])
    with pytest.raises(K.L.SALibraryError, match="storage type"):
        K.quant_affine(x, 0, 1.0, 0.0, -129, 127, q8)
    with pytest.raises(K.L.SALibraryError, match="mode"):
        K.quant_affine(x, 2, 1.0, 0.0, -128, 127, q8)
    with pytest.raises(K.L.SALibraryError, match="E4M3"):
        K.dequant_fp8(q8, 1.0, 8, 7, x)
