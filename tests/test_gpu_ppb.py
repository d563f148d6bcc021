"""sa_ppb_* on the GPU (PPBAggregator's kernels) against Python's own integers
written out here: ``a * b % m``, ``pow(a, e, m)`` and the one-line field
expression.  Every case is exact: integer for integer, float64 bit for bit."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import chacha_oracle as co  # noqa: E402
import gpu_copies as G  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PRIMES = json.load(open(os.path.join(HERE, "golden", "ppb_keys.json")))
BITS, BIAS, EXPAND = 55, 20.0, 10e12
SPECIAL = ("zero", "one", "minus_one", "ones")


def _key(K):
    from sfl_amd.security.aggregation.ppb_aggregator import PaillierKey

    return PaillierKey(int(PRIMES[str(K)]["p"], 16), int(PRIMES[str(K)]["q"], 16))


def _up(ints, count):
    """Python integers as rows of ``count`` limbs on the device."""
    raw = b"".join(int(v).to_bytes(4 * count, "little") for v in ints)
    return G._dev(np.frombuffer(raw, dtype=np.int32))


def _down(t, count):
    raw = G._host(t).tobytes()
    return [int.from_bytes(raw[at:at + 4 * count], "little") for at in range(0, len(raw), 4 * count)]


def _consts(key):
    return G._dev(key.consts().view(np.int32))


def _operands(key, C, rows, seed):
    """``C`` arrays of ``rows`` numbers below n^2: 0, 1, n^2 - 1 and the all-ones number reduced lead them."""
    import random

    rnd = random.Random(seed)
    planted = {"zero": 0, "one": 1, "minus_one": key.n2 - 1, "ones": ((1 << (2 * key.bits)) - 1) % key.n2}
    vals = [[rnd.randrange(key.n2) for _ in range(rows)] for _ in range(C)]
    for j in range(rows):
        vals[j % C][j] = planted[SPECIAL[j % 4]]
        if j % 8 >= 4:
            vals[(j + 1) % C][j] = planted[SPECIAL[(j // 8) % 4]]
    return vals


@pytest.mark.parametrize("rows", [1, 2, 67])
@pytest.mark.parametrize("C", [1, 2, 3, 8])
@pytest.mark.parametrize("K", [128, 512, 2048])
def test_add_is_the_product_mod_n2(K, C, rows):
    from sfl_amd import kernels as Kn

    key = _key(K)
    vals = _operands(key, C, rows, K + C + rows)
    out = torch.empty(rows * K // 16, dtype=Kn.LIMB, device=G.DEV)
    Kn.ppb_add([_up(v, K // 16) for v in vals], rows, K, _consts(key), out)
    want = []
    for j in range(rows):
        a = 1
        for v in vals:
            a = a * v[j] % key.n2
        want.append(a)
    assert _down(out, K // 16) == want


def _field(x, w=1.0, total=1.0):
    return int(abs(float(x) * w / total + BIAS) * EXPAND)


def _plain(xs, per_row, w=1.0, total=1.0):
    rows = []
    for at in range(0, len(xs), per_row):
        rows.append(int("".join(bin(_field(x, w, total))[2:].zfill(BITS) for x in xs[at:at + per_row]), 2))
    return rows


def _r(key_bytes, nonce, j, key):
    blocks = -(-key.bits // 512)
    for t in range(64):
        words = co.blocks(co.key_words(key_bytes), nonce, (64 * j + t) * blocks, blocks).reshape(-1)[:key.bits // 32]
        r = int.from_bytes(words.astype("<u4").tobytes(), "little")
        if 0 < r < key.n:
            return r, t
    raise AssertionError("no candidate")


@pytest.mark.parametrize("full,more", [(0, 1), (1, -1), (1, 0), (1, 1), (2, 1)])
@pytest.mark.parametrize("K,chacha", [(128, bytes(range(32))), (128, bytes([4]) * 32), (512, bytes(range(32))),
                                      (2048, bytes(range(32)))])
def test_encode_then_encrypt(K, chacha, full, more):
    """``full * per_row + more`` elements.  ``bytes([4]) * 32`` at K = 128: row 1's
    first candidate is above n, so its second is taken."""
    from sfl_amd import kernels as Kn

    key = _key(K)
    per_row = K // BITS
    n = full * per_row + more
    x = np.random.default_rng(n).uniform(-20, 20, n)
    rows, nonce = -(-n // per_row), 5
    flags = torch.zeros(1, dtype=Kn.LIMB, device=G.DEV)
    plain = torch.empty(rows * K // 32, dtype=Kn.LIMB, device=G.DEV)
    Kn.ppb_encode(G._dev(x), 2.0, 7.0, 3, BIAS, EXPAND, K, BITS, plain, flags)
    want = _plain(x, per_row, 2.0, 7.0)
    assert _down(plain, K // 32) == want
    ct = torch.empty(rows * K // 16, dtype=Kn.LIMB, device=G.DEV)
    Kn.ppb_encrypt(plain, rows, K, G._dev(key.consts(private=False).view(np.int32)), chacha, nonce, ct, flags)
    rs = [_r(chacha, nonce, j, key) for j in range(rows)]
    assert _down(ct, K // 16) == [(1 + m * key.n) * pow(r, key.n, key.n2) % key.n2 for m, (r, _) in zip(want, rs)]
    assert G._item(flags) == 0
    if chacha == bytes([4]) * 32 and rows > 1:
        assert rs[1][1] == 1


@pytest.mark.parametrize("K", [128, 512, 2048])
def test_decrypt_is_the_python_formula(K):
    from sfl_amd import kernels as Kn

    key = _key(K)
    rows = 67
    cts = _operands(key, 2, rows, K)[0]
    cts[8], cts[9] = key.encrypt(0, 12345), key.encrypt(key.n - 1, 54321)  # plaintexts 0 and n - 1
    out = torch.empty(rows * K // 32, dtype=Kn.LIMB, device=G.DEV)
    scratch = torch.empty(rows * K // 16, dtype=Kn.LIMB, device=G.DEV)
    Kn.ppb_decrypt(_up(cts, K // 16), rows, K, _consts(key), scratch, out)
    got = _down(out, K // 32)
    assert got == [(pow(c, key.lam, key.n2) - 1) // key.n * key.mu % key.n for c in cts]
    assert got[8] == 0 and got[9] == key.n - 1


def _edge_values(dtype):
    limit = ((1 << BITS) - 1) // 8
    top = np.float64(limit) / EXPAND - BIAS
    while _field(dtype(top)) > limit:
        top = np.nextafter(top, 0)
    if dtype is np.int64:
        return np.array([-20, 0, int(top), 5, -3, 17, 1], dtype)
    half = [np.nextafter(0.5, 0), 0.5, np.nextafter(0.5, 1), 0.5 - 2.0 ** -48, 0.5 + 2.0 ** -48]  # 20.5e13 is an integer
    vals = np.array([-20.0, 0.0, top] + half + [1 / 3, -19.999999], np.float64).astype(dtype)
    if _field(vals[2]) > limit:  # (float32 rounded the largest value up)
        vals[2] = np.nextafter(vals[2], dtype(0))
    return vals


@pytest.mark.parametrize("K", [128, 2048])
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int64])
def test_encode_and_decode(dtype, K):
    from sfl_amd import kernels as Kn

    x = _edge_values(dtype)
    per_row = K // BITS
    rows = -(-len(x) // per_row)
    flags = torch.zeros(1, dtype=Kn.LIMB, device=G.DEV)
    plain = torch.empty(rows * K // 32, dtype=Kn.LIMB, device=G.DEV)
    Kn.ppb_encode(G._dev(x), 1.0, 1.0, 8, BIAS, EXPAND, K, BITS, plain, flags)
    assert G._item(flags) == 0
    assert _down(plain, K // 32) == _plain(x, per_row)
    out = torch.empty(len(x), dtype=torch.float64, device=G.DEV)
    Kn.ppb_decode(plain, 8, BIAS, EXPAND, K, BITS, out)
    want = np.array([_field(v) / EXPAND - 8 * BIAS for v in x], np.float64)
    assert np.array_equal(G._bits(G._host(out)), G._bits(want))


@pytest.mark.parametrize("value,flag", [(-20.000001, 1), (float("nan"), 2), (431.0, 4)])
def test_encode_flags_the_refusals(value, flag):
    from sfl_amd import kernels as Kn

    x = np.array([1.0, value, 2.0])
    flags = torch.zeros(1, dtype=Kn.LIMB, device=G.DEV)
    plain = torch.empty(2 * 4, dtype=Kn.LIMB, device=G.DEV)
    Kn.ppb_encode(G._dev(x), 1.0, 1.0, 8, BIAS, EXPAND, 128, BITS, plain, flags)
    assert G._item(flags) == flag


@pytest.mark.parametrize("K,fallback", [(2048, 0), (192, 1)])
def test_average_end_to_end(K, fallback):
    """Bit-identical to the host form on the same inputs and keys, and within
    C * 2 / expand of np.average: one truncation per party of at most
    1 / expand, doubled for the float64 rounding of x * w / total."""
    from sfl_amd.device import PYU, PYUObject
    from sfl_amd.security.aggregation import PPBAggregator

    server = PYU("server", 0)
    p, q = (int(PRIMES[str(K)][k], 16) for k in "pq")
    rng = np.random.default_rng(K)
    data = [[rng.standard_normal(5), rng.standard_normal((3, 25))] for _ in range(3)]
    weights = [2.0, 3.0, 0.5]
    make = lambda: PPBAggregator.from_primes(server, [server] * 3, p, q,  # noqa: E731
                                             _party_keys=[bytes([i]) * 32 for i in range(3)])
    host, dev = make(), make()
    want = host.average([PYUObject(server, d) for d in data], axis=0, weights=weights).data
    got = dev.average([PYUObject(server, [G._dev(x).reshape(x.shape) for x in d]) for d in data], axis=0,
                      weights=weights).data
    assert dev.last_report["host_fallback"] == fallback
    for l, (a, b) in enumerate(zip(got, want)):
        assert a.is_cuda and a.dtype == torch.float64 and tuple(a.shape) == b.shape
        assert np.array_equal(G._bits(G._host(a)), G._bits(b))
        assert np.abs(b - np.average([d[l] for d in data], axis=0, weights=weights)).max() <= 3 * 2 / EXPAND
