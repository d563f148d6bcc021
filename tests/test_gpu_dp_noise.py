"""The DP pre-step's Gaussian noise on the GPU against a float64 reference
(oracle/dp.py gauss64): every one of 2^22 normals, their statistics, the
Box-Muller inputs where the hardware log / sin / cos units are at their
worst, the carry of the Philox block counter into its second word, in-place
use and the argument checks -- for the standalone kernel (sa_dp_perturb_f32)
and the fused one (sa_mask_dp), which must agree bit for bit.

With x = 0, noise_std = 1 and num_updates = 1 the standalone kernel returns
the normals themselves: 0 * scale + z * 1 * 1 (the exact-reciprocal path)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import dp_noise_stats as S  # noqa: E402
from gpu_copies import DEV, _dev, _host, _item, _u64  # noqa: E402
from oracle import dp as D  # noqa: E402
from oracle import secagg as o  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _K():
    from sfl_amd import kernels as K

    return K


def _L():
    from sfl_amd import _lib as L

    return L


def _sumsq(x):
    L = _L()
    out = torch.zeros(1, dtype=torch.float64, device=DEV)
    part = torch.empty(L.SA_DP_PARTIALS, dtype=torch.float64, device=DEV)
    return _K().sumsq_f32(x, out, part)


def _normals(key, counter0, n):
    """The standalone kernel's normals of elements counter0 .. counter0+n-1."""
    K = _K()
    s = _sumsq(torch.ones(4, device=DEV))
    dp = K.make_dp(s, l2_norm_clip=1.0, noise_std=1.0, num_updates=1, key=key, counter0=counter0)
    y = K.dp_perturb(torch.zeros(n, device=DEV), torch.full((n,), SENTINEL, device=DEV), dp)
    torch.cuda.synchronize()
    return _host(y)


def _streams(nstreams):
    L = _L()
    seeds = [o.pair_seed(0, j + 1) for j in range(nstreams)]
    return seeds, [(L.pcg64_from_seed(sd), 1 if j % 2 else -1, j) for j, sd in enumerate(seeds)]


def _within(z, z64):
    return np.abs(np.asarray(z, dtype=np.float64) - z64) <= S.RTOL * np.abs(z64) + S.ATOL


@pytest.fixture(scope="module")
def device_streams():
    """2^22 device normals of S.KEY at counter 0, of S.KEY + 1 at the same
    counters, and of S.KEY's next window (three launches, read-only)."""
    out = tuple(_normals(k, c, S.N) for k, c in ((S.KEY, 0), (S.KEY + 1, 0), (S.KEY, S.N)))
    for z in out:
        z.setflags(write=False)
    return out


def test_every_normal_within_tolerance_of_float64_reference(device_streams):
    """All 2^22 normals of the standalone kernel against gauss64, element by
    element: |z - z64| <= 2e-5 |z64| + 2e-6; and against the float32
    restatement gauss, the suite's earlier check, at 40 times its size."""
    z = device_streams[0]
    assert z.dtype == np.float32 and z.size == S.N and np.all(np.isfinite(z))
    z64 = D.gauss64(S.KEY, 0, S.N)
    used = np.abs(z.astype(np.float64) - z64) / (S.RTOL * np.abs(z64) + S.ATOL)
    print(f"device vs gauss64: max |error| {float(np.abs(z - z64).max()):.3g}, {float(used.max()):.4f} of the "
          f"tolerance at element {int(used.argmax())}")
    msg = S.worst_element(z, z64, S.stream_words_of(S.KEY, 0))
    assert not msg, msg
    assert np.allclose(z, D.gauss(S.KEY, 0, S.N), rtol=S.RTOL, atol=S.ATOL)


def test_noise_statistics_of_the_device_stream(device_streams):
    """Moments, CDF, tails, autocorrelation of the device's 2^22 normals and
    their correlation with another key's and the next window's, each within
    its formula bound (tests/dp_noise_stats.py)."""
    z, zk, zn = device_streams
    assert not np.array_equal(z, zk) and not np.array_equal(z, zn)
    S.check_noise_statistics(S.noise_statistics(z, zk, zn), "device")


def _fused_vs_perturb_then_mask(x, key, counter0, updates, nstreams=3, noise_std=1.0):
    """sa_mask_dp against sa_dp_perturb_f32 + sa_mask bit for bit (masked
    vector and digest) and against the oracle's quantize + mask streams of
    the perturbed input; returns the perturbed input (host float32)."""
    K = _K()
    n = x.numel()
    s = _sumsq(x)
    seeds, streams = _streams(nstreams)
    mk = lambda: K.make_dp(s, l2_norm_clip=0.3, noise_std=noise_std, num_updates=updates, key=key,  # noqa: E731
                           counter0=counter0)
    xp = K.dp_perturb(x, torch.empty_like(x), mk())
    m1 = torch.empty(n, dtype=torch.int64, device=DEV)
    d1 = torch.zeros(1, dtype=torch.int64, device=DEV)
    K.mask(xp, m1, streams, weight=3.0, digest=d1)
    m2 = torch.empty(n, dtype=torch.int64, device=DEV)
    d2 = torch.zeros(1, dtype=torch.int64, device=DEV)
    K.mask_dp(x, m2, streams, mk(), weight=3.0, digest=d2)
    torch.cuda.synchronize()
    bad = (m1 != m2).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} masked elements differ, first {_host(bad[:8]).tolist()}"
    assert torch.equal(d1, d2)
    xph = _host(xp)
    exp = o.quantize(xph, 3)
    for sd, (_, sg, _) in zip(seeds, streams):
        mm = o.mask_stream(sd, n)
        exp = exp + mm if sg > 0 else exp - mm
    assert np.array_equal(_u64(m2), exp)
    return xph, D.clip_scale(_item(s), 0.3)


def _fused_normals(key, counter0, n):
    """The fused kernel's own normals: x = 0, noise_std = 1, num_updates = 1,
    no mask stream, 40 fraction bits -> trunc(z 2^40), exact for a float32
    |z| >= 2^-17 and within 2^-40 below."""
    K = _K()
    s = _sumsq(torch.ones(4, device=DEV))
    dp = K.make_dp(s, l2_norm_clip=1.0, noise_std=1.0, num_updates=1, key=key, counter0=counter0)
    m = torch.empty(n, dtype=torch.int64, device=DEV)
    K.mask_dp(torch.zeros(n, device=DEV), m, [], dp, weight=1.0, fxp_bits=40)
    torch.cuda.synchronize()
    return _host(m)


EXTREME_IDS = [f"{e[0].split(' (')[0]} @ {e[1]}".replace(" ", "") for e in S.EXTREMES]


@pytest.mark.parametrize("name,blk,j,which,val", S.EXTREMES, ids=EXTREME_IDS)
def test_extreme_inputs_standalone(name, blk, j, which, val):
    """The Philox blocks whose words put u1 at 2^-24 or 1, or u2 at 0, next
    to a quarter turn, on one, or at 1 - 2^-24 (where cos or sin crosses zero
    and an approximate unit's relative error is unbounded): all four normals
    finite and within the tolerance of gauss64.  Joint extremes (probability
    2^-48 per pair) are out of reach."""
    z = _normals(S.KEY, 4 * blk, 4)
    z64 = D.gauss64(S.KEY, 4 * blk, 4)
    w = D.philox_words(S.KEY, 4 * blk, 4)[0]
    print(f"{name}: block {blk} words {[hex(int(v)) for v in w]} device {z.tolist()} float64 {z64.tolist()}")
    assert np.all(np.isfinite(z)), (name, z)
    assert np.all(_within(z, z64)), (name, z.tolist(), z64.tolist(), [hex(int(v)) for v in w])


@pytest.mark.parametrize("updates", [4, 3])
def test_extreme_inputs_fused_equals_perturb_then_mask(updates):
    """The same blocks through sa_mask_dp (a small non-zero x, weight 3.0,
    three streams; the extreme block between two ordinary ones): bit for bit
    perturb-then-mask and the oracle's masked vector of the perturbed input,
    whose noise is gauss64's within the tolerance; the fused kernel's own
    normals there (read back through 40 fraction bits) are the standalone
    kernel's."""
    for name, blk, j, which, val in S.EXTREMES:
        c0 = 4 * (blk - 1)
        x = _dev(np.array([0.01, -0.02, 0.03, 0.005, -0.015, 0.025, 0.02, -0.01, 0.004, -0.03, 0.011, 0.007],
                          np.float32))
        xp, scale = _fused_vs_perturb_then_mask(x, S.KEY, c0, updates)
        z64 = D.gauss64(S.KEY, c0, 12)
        noise = (xp.astype(np.float64) - (_host(x) * scale).astype(np.float64)) * updates
        # x * scale + z / updates in float32: two roundings of values below 8 on top of the normal's tolerance
        assert np.all(np.abs(noise - z64) <= S.RTOL * np.abs(z64) + S.ATOL + updates * 8 * 2.0**-23), (name, blk)
        zs = _normals(S.KEY, c0, 12)
        zf = _fused_normals(S.KEY, c0, 12)
        assert np.array_equal(zf.view(np.uint64), o.quantize(zs, None, 40)), (name, blk, zs.tolist())
        assert np.all(np.abs(zf / 2.0**40 - z64) <= S.RTOL * np.abs(z64) + S.ATOL + 2.0**-40), (name, blk)


@pytest.mark.parametrize("b0", [(1 << 32) - 3, (1 << 40) + 5])
def test_block_counter_carries_into_the_second_word(b0):
    """counter0 = 4 b0, n = 37: at b0 = 2^32 - 3 blocks 2^32-3 .. 2^32+6 cross
    from Philox counter word 0 into word 1; at 2^40 + 5 word 1 is non-zero
    throughout.  The standalone and the fused kernel index their blocks with
    their own code: each against gauss64 / gauss, and against each other
    bit for bit."""
    n, c0 = 37, 4 * b0
    z64 = D.gauss64(S.KEY, c0, n)
    z32 = D.gauss(S.KEY, c0, n)
    # word 1 matters: the stream of the block numbers cut to 32 bits is another one from block 2^32 on
    cut = np.concatenate([D.gauss64(S.KEY, 4 * ((b0 + i) & 0xFFFFFFFF), 4) for i in range(10)])[:n]
    assert not np.allclose(z64[12:], cut[12:], atol=0.1)
    z = _normals(S.KEY, c0, n)
    msg = S.worst_element(z, z64, S.stream_words_of(S.KEY, c0))
    assert not msg, msg
    assert np.allclose(z, z32, rtol=S.RTOL, atol=S.ATOL)
    zf = _fused_normals(S.KEY, c0, n)
    assert np.array_equal(zf.view(np.uint64), o.quantize(z, None, 40))
    assert np.all(np.abs(zf / 2.0**40 - z64) <= S.RTOL * np.abs(z64) + S.ATOL + 2.0**-40)
    assert np.allclose(zf / 2.0**40, z32, rtol=S.RTOL, atol=S.ATOL + 2.0**-40)
    for updates in (8, 3):
        x = torch.randn(n, device=DEV, generator=torch.Generator(DEV).manual_seed(b0 % 1000)) * 0.05
        _fused_vs_perturb_then_mask(x, S.KEY, c0, updates, noise_std=0.25)


@pytest.mark.parametrize("n", [1, 5, 1023, 1025, 4097, 262_147])
def test_perturb_in_place_equals_out_of_place(n):
    """sa_dp_perturb_f32 with out aliasing x (include/sfl_sa.h allows it)
    equals the out-of-place result bit for bit; nothing past n is written."""
    K = _K()
    buf = torch.full((n + 16,), SENTINEL, device=DEV)
    buf[:n] = torch.randn(n, device=DEV, generator=torch.Generator(DEV).manual_seed(n)) * 0.2
    x = buf[:n].clone()
    s = _sumsq(x)
    for updates in (4, 3):
        mk = lambda: K.make_dp(s, l2_norm_clip=0.5, noise_std=0.3, num_updates=updates, key=S.KEY,  # noqa: E731
                               counter0=4 * 11)
        y = K.dp_perturb(x, torch.empty_like(x), mk())
        b = buf.clone()
        K.dp_perturb(b[:n], b[:n], mk())
        torch.cuda.synchronize()
        assert torch.equal(b[:n].view(torch.int32), y.view(torch.int32))
        assert torch.all(b[n:] == SENTINEL)
        assert not torch.equal(y, x)


def test_bad_arguments_are_refused_before_any_launch():
    """x or out 4 bytes into an allocation, num_updates = 0 and a counter0
    that is no multiple of 4 (set on the struct, past make_dp's own check):
    SA_ERR_ARG through L.check, and the output keeps its sentinel."""
    K, L = _K(), _L()
    n = 64
    s = _sumsq(torch.ones(4, device=DEV))
    good = lambda **kw: K.make_dp(s, **{**dict(l2_norm_clip=1.0, noise_std=1.0, num_updates=2, key=1), **kw})  # noqa: E731
    xbuf = torch.ones(n + 4, device=DEV)
    obuf = torch.full((n + 4,), SENTINEL, device=DEV)
    assert xbuf.data_ptr() % 16 == 0 and obuf.data_ptr() % 16 == 0
    odd = good()
    odd.counter0 = 6
    with pytest.raises(ValueError):
        good(counter0=6)
    cases = [("x at +4 bytes", xbuf[1:n + 1], obuf[:n], good()), ("out at +4 bytes", xbuf[:n], obuf[1:n + 1], good()),
             ("num_updates = 0", xbuf[:n], obuf[:n], good(num_updates=0)), ("counter0 = 6", xbuf[:n], obuf[:n], odd)]
    for what, x, out, dp in cases:
        with pytest.raises(L.SALibraryError, match=f"code {L.SA_ERR_ARG}:"):
            K.dp_perturb(x, out, dp)
        torch.cuda.synchronize()
        assert torch.all(obuf == SENTINEL), what
    # the fused kernel shares the sa_dp check
    m = torch.full((n,), 77, dtype=torch.int64, device=DEV)
    for what, dp in (("num_updates = 0", good(num_updates=0)), ("counter0 = 6", odd)):
        with pytest.raises(L.SALibraryError, match=f"code {L.SA_ERR_ARG}:"):
            K.mask_dp(xbuf[:n], m, _streams(3)[1], dp, weight=3.0)
        torch.cuda.synchronize()
        assert torch.all(m == 77), what
    # and the good arguments do run
    K.dp_perturb(xbuf[:n], obuf[:n], good())
    torch.cuda.synchronize()
    assert torch.all(obuf[:n] != SENTINEL) and torch.all(obuf[n:] == SENTINEL)
