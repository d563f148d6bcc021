"""The secure DP noise on the GPU (sfl_amd/csrc/sa_dp_secure.hip): the ChaCha20
keystream bit for bit against the numpy restatement (tests/chacha_oracle.py),
the Holohan-Braghin transform at its edge inputs, the perturb kernel bit for
bit against the device's own keystream + transform and within the project's
noise tolerance of the restatement, the statistics of 2^22 device normals,
the argument checks, and SecureGaussianModelDP.__call__.

Every array moves through tests/gpu_copies.py (pinned buffers)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import chacha_oracle as co  # noqa: E402
import dp_noise_stats as S  # noqa: E402
from gpu_copies import DEV, _dev, _host  # noqa: E402
from oracle import dp as D  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
CANARY = 0x5A5A5A5A
KEY_A, KEY_B, NONCE = bytes(range(32)), bytes(range(1, 33)), 7


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


def _sumsq(x, out=None):
    """x's squared norm on the device (added to ``out`` when given)."""
    L = _L()
    part = torch.empty(L.SA_DP_PARTIALS, dtype=torch.float64, device=DEV)
    if out is None:
        return _K().sumsq_f32(x, torch.zeros(1, dtype=torch.float64, device=DEV), part)
    return _K().sumsq_f32(x, out, part, accumulate=True)


def _keystream(key, nonce, b0, nb):
    """(device int32 words with 16 canary words behind, host (nb, 16) uint32)."""
    buf = torch.full((16 * nb + 16,), CANARY, dtype=torch.int32, device=DEV)
    _K().chacha20_keystream(key, nonce, b0, buf[:16 * nb])
    torch.cuda.synchronize()
    h = _host(buf).view(np.uint32)
    assert np.all(h[16 * nb:] == CANARY), "the keystream kernel wrote past its last block"
    return buf[:16 * nb], h[:16 * nb].reshape(nb, 16)


def _device_normals64(key, nonce, counter0, n, sigma):
    """The device's own z64 of noise indices counter0 .. counter0 + n - 1:
    sa_hb_normals_f64 of sa_chacha20_keystream."""
    nb = (n + 3) // 4
    words, _ = _keystream(key, nonce, counter0 // 4, nb)
    z = _K().hb_normals(words, sigma, torch.empty(4 * nb, dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()
    return _host(z)[:n]


def _within(z, z64):
    return np.abs(np.asarray(z, dtype=np.float64) - z64) <= S.RTOL * np.abs(z64) + S.ATOL


def _words_of(u1_m, u2_m, low=0):
    """Words a, b, c, d whose uniforms are u1_m / 2^53 and u2_m / 2^53; ``low``
    fills the 11 bits below each mantissa, which the transform must ignore."""
    v1, v2 = (int(u1_m) << 11) | low, (int(u2_m) << 11) | low
    return [v1 & 0xFFFFFFFF, v1 >> 32, v2 & 0xFFFFFFFF, v2 >> 32]


# ---------------------------------------------------------------- keystream

@pytest.mark.parametrize("b0", [0, (1 << 32) - 3, (1 << 40) + 5], ids=["0", "2^32-3", "2^40+5"])
@pytest.mark.parametrize("nb", [1, 255, 256, 257, 1025])
def test_keystream_equals_the_restatement_bit_for_bit(nb, b0):
    _, got = _keystream(KEY_A, NONCE, b0, nb)
    exp = co.blocks(co.key_words(KEY_A), NONCE, b0, nb)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {nb} blocks differ, first {bad[:4].tolist()}"


def test_keystream_depends_on_key_nonce_and_both_counter_words():
    base = _keystream(KEY_A, NONCE, 5, 3)[1]
    for what, key, nonce, b0 in (("key", KEY_B, NONCE, 5), ("nonce low", KEY_A, NONCE + 1, 5),
                                 ("nonce high", KEY_A, NONCE + (1 << 32), 5), ("counter high", KEY_A, NONCE, 5 + (1 << 32))):
        got = _keystream(key, nonce, b0, 3)[1]
        assert not np.array_equal(got, base), what
        assert np.array_equal(got, co.blocks(co.key_words(key), nonce, b0, 3)), what
    assert np.array_equal(_keystream(KEY_A, NONCE, 6, 2)[1], base[1:])
    assert np.array_equal(_keystream(KEY_A, NONCE, 5, 3)[1], _L().chacha20_blocks_host(KEY_A, NONCE, 5, 3))


# ---------------------------------------------------------------- transform

def _edge_words():
    top = (1 << 53) - 1
    u1s = [0, 1 << 50, 3 << 50, (3 << 50) - 1, (3 << 50) + 1, 7 << 50, (7 << 50) - 1, (7 << 50) + 1, top]
    u2s = [0, top, 1, 1 << 52, top - 1]
    rows = [_words_of(a, b, low) for a in u1s for b in u2s for low in (0, 0x7FF)]
    return np.array(rows, dtype=np.uint32)


@pytest.mark.parametrize("sigma", [1.0, 0.3])
def test_transform_at_its_edge_inputs_and_on_random_words(sigma):
    """u2 = 0 (r = 0) and 1 - 2^-53 (the largest radius, 8.57); u1 = 0, 1/8,
    3/8 and 7/8 (where sin + cos cancels) and their neighbours, 1 - 2^-53;
    then 2^16 random word quadruples: every normal finite and, cast to
    float32, within RTOL |z_ref| + ATOL of the numpy restatement."""
    K = _K()
    edge = _edge_words()
    rnd = np.random.default_rng(53).integers(0, 1 << 32, (1 << 16, 4), dtype=np.uint64).astype(np.uint32)
    words = np.concatenate([edge, rnd])
    n = words.shape[0]
    buf = torch.full((n + 8,), SENTINEL, dtype=torch.float64, device=DEV)
    K.hb_normals(_dev(words.view(np.int32)), sigma, buf[:n])
    torch.cuda.synchronize()
    h = _host(buf)
    z, ref = h[:n], co.normals_of_words(words, sigma)
    assert np.all(h[n:] == SENTINEL)
    assert np.all(np.isfinite(z)) and np.all(np.isfinite(ref))
    u1, u2 = co.uniforms(edge)
    assert np.all(z[:edge.shape[0]][u2 == 0.0] == 0.0)
    assert float(np.abs(z).max()) <= sigma * 8.58 * np.sqrt(2.0)
    err = np.abs(z - ref)
    z32, ref32 = z.astype(np.float32), ref.astype(np.float32)
    print(f"sigma {sigma}: float64 max |z_dev - z_numpy| = {float(err.max()):.3g} (edge rows {float(err[:edge.shape[0]].max()):.3g}); "
          f"float32 casts differ in {int((z32[edge.shape[0]:] != ref32[edge.shape[0]:]).sum())} of {rnd.shape[0]} random "
          f"and {int((z32[:edge.shape[0]] != ref32[:edge.shape[0]]).sum())} of {edge.shape[0]} edge elements")
    bad = np.nonzero(~_within(z32, ref))[0]
    assert bad.size == 0, (bad[:4].tolist(), words[bad[:4]].tolist(), z[bad[:4]].tolist(), ref[bad[:4]].tolist())
    # the 11 bits below each 53-bit mantissa are not part of the uniforms
    k = edge.shape[0]
    assert np.array_equal(z[0:k:2].view(np.uint64), z[1:k:2].view(np.uint64))


# ---------------------------------------------------------------- perturb

def _expected(x, scale, key, nonce, counter0, sigma, updates):
    """(the output sa_dp_perturb_secure_f32 must give bit for bit:
    fl32(x * scale) + fl32(fl32(z64_dev) / updates) with the device's own
    z64; the restatement's z64; the bound of |output - the same formula on
    the restatement's z64|: the noise tolerance over updates plus the three
    float32 roundings behind it)."""
    n = x.size
    z_dev = _device_normals64(key, nonce, counter0, n, sigma)
    z_ref = co.normals64(co.key_words(key), nonce, counter0, n, sigma)
    u = np.float32(updates)
    exp = x * np.float32(scale) + z_dev.astype(np.float32) / u
    ref = x * np.float32(scale) + z_ref.astype(np.float32) / u
    assert exp.dtype == np.float32
    tol = (S.RTOL * np.abs(z_ref) + S.ATOL) / updates + 2.0**-23 * (np.abs(x * np.float32(scale)) + np.abs(z_ref) / updates)
    return exp, ref.astype(np.float64), tol


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 4099])
def test_perturb_equals_keystream_transform_and_clip(n):
    """Tail, one tile, a tile + 1, several tiles; num_updates 4 (a power of
    two) and 3; with and without the per-layer norm; out of place and in
    place (out aliasing x); nothing past n written."""
    K = _K()
    rng = np.random.default_rng(n)
    xh = (rng.standard_normal(n) * 0.2).astype(np.float32)
    other = (rng.standard_normal(33) * 0.2).astype(np.float32)
    x = _dev(xh)
    lay = _sumsq(x)
    total = _sumsq(_dev(other), _sumsq(x))
    torch.cuda.synchronize()
    lay_h, total_h = float(_host(lay)[0]), float(_host(total)[0])
    assert lay_h == float(D.layer_sq_norm(xh)) and total_h == float(D.global_sq([xh, other]))
    clip, sigma, c0 = 0.5, 0.3, 4 * 11
    for updates in (4, 3):
        for layer in (None, lay):
            mk = lambda: K.make_dp_secure(total, l2_norm_clip=clip, noise_std=sigma, num_updates=updates,  # noqa: E731
                                          key=KEY_A, nonce=NONCE, counter0=c0, sumsq_layer=layer)
            obuf = torch.full((n + 16,), SENTINEL, device=DEV)
            K.dp_perturb_secure(x, obuf[:n], mk())
            ibuf = torch.full((n + 16,), SENTINEL, device=DEV)
            ibuf[:n].copy_(x)
            K.dp_perturb_secure(ibuf[:n], ibuf[:n], mk())
            torch.cuda.synchronize()
            out, inp = _host(obuf), _host(ibuf)
            scale = D.clip_scale(total_h, clip, None if layer is None else lay_h)
            exp, ref, tol = _expected(xh, scale, KEY_A, NONCE, c0, sigma, updates)
            what = (n, updates, layer is not None)
            assert np.all(out[n:] == SENTINEL) and np.all(inp[n:] == SENTINEL), what
            bad = np.nonzero(out[:n].view(np.uint32) != exp.view(np.uint32))[0]
            assert bad.size == 0, (what, bad[:4].tolist(), out[bad[:4]].tolist(), exp[bad[:4]].tolist())
            assert np.array_equal(inp[:n].view(np.uint32), out[:n].view(np.uint32)), what
            assert np.all(np.abs(out[:n].astype(np.float64) - ref) <= tol), what
            assert not np.array_equal(out[:n], xh * np.float32(scale)), what


def _normals(key, nonce, counter0, n):
    """The perturb kernel's normals themselves: x = 0, sigma = 1, num_updates = 1."""
    K = _K()
    s = _sumsq(_dev(np.ones(4, dtype=np.float32)))
    dp = K.make_dp_secure(s, l2_norm_clip=1.0, noise_std=1.0, num_updates=1, key=key, nonce=nonce, counter0=counter0)
    y = K.dp_perturb_secure(torch.zeros(n, device=DEV), torch.full((n,), SENTINEL, device=DEV), dp)
    torch.cuda.synchronize()
    return _host(y)


def test_block_counter_carries_into_word_13():
    """counter0 = 4 (2^32 - 3), n = 37: blocks 2^32 - 3 .. 2^32 + 6."""
    n, c0 = 37, 4 * ((1 << 32) - 3)
    z = _normals(KEY_A, NONCE, c0, n)
    ref = co.normals64(co.key_words(KEY_A), NONCE, c0, n, 1.0)
    cut = co.normals64(co.key_words(KEY_A), NONCE, 0, n, 1.0)[12:]  # the stream of a counter cut to 32 bits
    assert not np.allclose(ref[12:], cut, atol=0.1)
    assert np.all(np.isfinite(z)) and np.all(_within(z, ref))
    assert np.array_equal(z, _device_normals64(KEY_A, NONCE, c0, n, 1.0).astype(np.float32))


def test_key_nonce_and_window_each_change_the_noise():
    n = 64
    base = _normals(KEY_A, NONCE, 0, n)
    others = {"key": _normals(KEY_B, NONCE, 0, n), "nonce": _normals(KEY_A, NONCE + 1, 0, n),
              "window": _normals(KEY_A, NONCE, n, n)}
    for what, z in others.items():
        assert not np.any(z == base), what
    assert np.array_equal(_normals(KEY_A, NONCE, 0, 2 * n)[n:], others["window"])


# ---------------------------------------------------------------- statistics

@pytest.fixture(scope="module")
def device_streams():
    """2^22 device normals of KEY_A at counter 0, of KEY_B at the same
    counters, and of KEY_A's next window (three launches, read-only)."""
    out = tuple(_normals(k, NONCE, c, S.N) for k, c in ((KEY_A, 0), (KEY_B, 0), (KEY_A, S.N)))
    for z in out:
        z.setflags(write=False)
    return out


def test_every_device_normal_within_tolerance_of_the_restatement(device_streams):
    z = device_streams[0]
    assert z.dtype == np.float32 and z.size == S.N and np.all(np.isfinite(z))
    ref = co.normals64(co.key_words(KEY_A), NONCE, 0, S.N, 1.0)
    used = np.abs(z.astype(np.float64) - ref) / (S.RTOL * np.abs(ref) + S.ATOL)
    print(f"device vs restatement: {float(used.max()):.4f} of the tolerance at element {int(used.argmax())}; "
          f"{int((z != ref.astype(np.float32)).sum())} of {S.N} float32 normals differ from numpy's")
    assert float(used.max()) <= 1.0


def test_noise_statistics_of_the_device_stream(device_streams):
    z, zk, zn = device_streams
    assert not np.array_equal(z, zk) and not np.array_equal(z, zn)
    S.check_noise_statistics(S.noise_statistics(z, zk, zn), "device")


# ---------------------------------------------------------------- refusals

def test_bad_arguments_are_refused_before_any_launch():
    """x or out 4 bytes into an allocation, num_updates = 0, counter0 = 6 (set
    on the struct, past make_dp_secure's own check) and a null sumsq:
    SA_ERR_ARG, and the output keeps its sentinel."""
    K, L = _K(), _L()
    n = 64
    s = _sumsq(_dev(np.ones(4, dtype=np.float32)))
    good = lambda **kw: K.make_dp_secure(s, **{**dict(l2_norm_clip=1.0, noise_std=1.0, num_updates=2, key=KEY_A,  # noqa: E731
                                                       nonce=NONCE), **kw})
    xbuf = torch.ones(n + 4, device=DEV)
    obuf = torch.full((n + 4,), SENTINEL, device=DEV)
    assert xbuf.data_ptr() % 16 == 0 and obuf.data_ptr() % 16 == 0
    odd = good()
    odd.counter0 = 6
    nosum = good()
    nosum.sumsq = None
    with pytest.raises(ValueError):
        good(counter0=6)
    with pytest.raises(ValueError):
        good(key=bytes(16))
    cases = [("x at +4 bytes", xbuf[1:n + 1], obuf[:n], good()), ("out at +4 bytes", xbuf[:n], obuf[1:n + 1], good()),
             ("num_updates = 0", xbuf[:n], obuf[:n], good(num_updates=0)), ("counter0 = 6", xbuf[:n], obuf[:n], odd),
             ("null sumsq", xbuf[:n], obuf[:n], nosum)]
    for what, x, out, dp in cases:
        with pytest.raises(L.SALibraryError, match=f"code {L.SA_ERR_ARG}:"):
            K.dp_perturb_secure(x, out, dp)
        torch.cuda.synchronize()
        assert torch.all(obuf == SENTINEL), what
    K.dp_perturb_secure(xbuf[:n], obuf[:n], good())
    torch.cuda.synchronize()
    assert torch.all(obuf[:n] != SENTINEL) and torch.all(obuf[n:] == SENTINEL)


# ---------------------------------------------------------------- the class

@pytest.mark.parametrize("each_layer", [False, True])
def test_secure_gaussian_model_dp_call(each_layer):
    """A two-layer list, numpy in -> numpy out and torch in -> torch out: each
    layer equals the kernel-level expectation at its own counter; a second
    call continues the counter."""
    from sfl_amd.security.privacy import SecureGaussianModelDP

    rng = np.random.default_rng(9)
    layers = [(rng.standard_normal((3, 5)) * 0.4).astype(np.float32), (rng.standard_normal(7) * 0.4).astype(np.float32)]
    clip, mult, updates = 0.7, 0.6, 3
    sigma = mult * clip * clip
    total = D.global_sq(layers)

    def expect(counter):
        out = []
        for a in layers:
            scale = D.clip_scale(total, clip, D.layer_sq_norm(a) if each_layer else None)
            out.append(_expected(a.reshape(-1), scale, KEY_B, NONCE, counter, sigma, updates)[0].reshape(a.shape))
            counter += -(-a.size // 4) * 4
        return out, counter

    m = SecureGaussianModelDP(mult, 8, num_updates=updates, l2_norm_clip=clip, is_clip_each_layer=each_layer,
                              device=DEV, key=KEY_B, nonce=NONCE)
    assert m.global_norm(layers) == float(np.sqrt(total))
    got = m(layers)
    exp, c1 = expect(0)
    assert c1 == 24 and m.counter == 24
    for g, e in zip(got, exp):
        assert isinstance(g, np.ndarray) and g.dtype == np.float32 and g.shape == e.shape
        assert np.array_equal(g.view(np.uint32), e.view(np.uint32))
    got = m([_dev(a).reshape(a.shape) for a in layers])  # the second call: torch in, the counter goes on
    exp2, c2 = expect(c1)
    assert c2 == 48 and m.counter == 48
    for g, e, first in zip(got, exp2, exp):
        assert isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.float32 and tuple(g.shape) == e.shape
        assert np.array_equal(_host(g).view(np.uint32), e.view(np.uint32))
        assert not np.array_equal(e, first)
