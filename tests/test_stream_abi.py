"""What the streaming entries (sa_sum_u64, sa_decode, sa_sum_f64; sa_sumsq_f32,
sa_dp_perturb_f32, sa_mask_dp's own checks; sa_dp_perturb_secure_f32,
sa_chacha20_keystream, sa_hb_normals_f64) refuse before any launch, without a
GPU: for every class of argument an entry checks, the return code and the
full text of sa_last_error().  The addresses below are never dereferenced:
every call is either refused or, with nothing to do, returns before a
launch."""
import ctypes as C

from sfl_amd import _lib as L
from test_compress_abi import refused

# distinct 16-byte aligned addresses, and ones that are 8-, 4-, 2- and 1-byte aligned only
A, B, OUT, SUMSQ, PART = (0x1000 * k for k in range(1, 6))
MISALIGNED = (0x1008, 0x1004, 0x1002, 0x1001)

# the tile kernels take one block per 256 lanes and a grid of at most 2^31 - 1 blocks:
# the smallest counts of lane items (and some larger ones) that no grid covers
LANES_TOO_MANY = ((2**31 - 1) * 256 + 1, 2**39, 2**39 + 1, 2**50)
# the server kernels: one lane per 4 pairs of 8-byte elements
SERVER_TOO_MANY = (2**42 - 2046, 2**42 - 2045, 2**42, 2**63, 2**64 - 1)
# the DP kernels: one lane per 4 float32 elements (the last block may be partial)
DP_TOO_MANY = (2**41 - 1023, 2**41 - 1020, 2**41, 2**50 + 1)


def ptrs(*addresses):
    return (C.c_void_p * len(addresses))(*addresses)


# ---------------------------------------------------------------------------
# sa_sum_u64, sa_decode, sa_sum_f64
# ---------------------------------------------------------------------------
def server_launch(n):
    return f"vector of {n} elements exceeds one server-kernel launch"


def test_sum_u64():
    lib = L.lib()
    for k in (0, -1, -7):
        refused(lib.sa_sum_u64(ptrs(A, B), k, 64, OUT, None), f"sa_sum_u64: bad arguments (k={k})")
        refused(lib.sa_sum_u64(ptrs(A, B), k, 0, OUT, None), f"sa_sum_u64: bad arguments (k={k})")
    refused(lib.sa_sum_u64(None, 2, 64, OUT, None), "sa_sum_u64: bad arguments (k=2)")
    refused(lib.sa_sum_u64(ptrs(A, B), 2, 64, None, None), "sa_sum_u64: bad arguments (k=2)")
    refused(lib.sa_sum_u64(ptrs(None, B), 2, 64, OUT, None), "sa_sum_u64: input 0 null or not 16-byte aligned")
    refused(lib.sa_sum_u64(ptrs(A, None), 2, 64, OUT, None), "sa_sum_u64: input 1 null or not 16-byte aligned")
    for bad in MISALIGNED:
        refused(lib.sa_sum_u64(ptrs(A, B, bad), 3, 64, OUT, None), "sa_sum_u64: input 2 null or not 16-byte aligned")
        refused(lib.sa_sum_u64(ptrs(bad, bad), 2, 64, OUT, None), "sa_sum_u64: input 0 null or not 16-byte aligned")
        refused(lib.sa_sum_u64(ptrs(A, B), 2, 64, bad, None), "sa_sum_u64: out not 16-byte aligned")
        refused(lib.sa_sum_u64(ptrs(A, bad), 2, 64, bad, None), "sa_sum_u64: input 1 null or not 16-byte aligned")
    for n in SERVER_TOO_MANY:
        refused(lib.sa_sum_u64(ptrs(A, B), 2, n, OUT, None), server_launch(n))
        refused(lib.sa_sum_u64(ptrs(A), 1, n, A, None), server_launch(n))  # out may alias in[0]
        refused(lib.sa_sum_u64(ptrs(*[A] * 40), 40, n, OUT, None), server_launch(n))  # a chain's first launch
        refused(lib.sa_sum_u64(ptrs(A, 0x1008), 2, n, OUT, None),
                "sa_sum_u64: input 1 null or not 16-byte aligned")  # the operands first
    assert lib.sa_sum_u64(None, 1, 0, None, None) == L.SA_OK  # empty vectors: their pointers may be null
    assert lib.sa_sum_u64(ptrs(0x1001), 1, 0, 0x1001, None) == L.SA_OK


def test_decode():
    lib = L.lib()
    for fxp in (-1, 63, 64, -2**31):
        refused(lib.sa_decode(A, 64, fxp, 1.0, None, OUT, None), "sa_decode: bad arguments")
        refused(lib.sa_decode(A, 0, fxp, 1.0, None, OUT, None), "sa_decode: bad arguments")  # even of nothing
    refused(lib.sa_decode(None, 64, 18, 1.0, None, OUT, None), "sa_decode: bad arguments")
    refused(lib.sa_decode(A, 64, 18, 1.0, None, None, None), "sa_decode: bad arguments")
    refused(lib.sa_decode(None, 64, 18, 1.0, B, None, None), "sa_decode: bad arguments")
    for n in SERVER_TOO_MANY:  # 16-byte aligned operands take the tile grid
        refused(lib.sa_decode(A, n, 18, 1.0, None, OUT, None), server_launch(n))
        refused(lib.sa_decode(A, n, 0, 2.0, B, OUT, None), server_launch(n))
        refused(lib.sa_decode(A, n, 62, 2.0, B, A, None), server_launch(n))
        refused(lib.sa_decode(A, n, 63, 2.0, B, OUT, None), "sa_decode: bad arguments")
    for fxp in (0, 18, 62):
        assert lib.sa_decode(None, 0, fxp, 1.0, None, None, None) == L.SA_OK
    assert lib.sa_decode(0x1001, 0, 18, 1.0, 0x1001, 0x1001, None) == L.SA_OK


def test_sum_f64():
    lib = L.lib()
    refused(lib.sa_sum_f64(None, 2, 64, OUT, None), "sa_sum_f64: bad arguments")
    refused(lib.sa_sum_f64(ptrs(A, B), 2, 64, None, None), "sa_sum_f64: bad arguments")
    for k in (0, -1):
        refused(lib.sa_sum_f64(ptrs(A, B), k, 64, OUT, None), "sa_sum_f64: bad arguments")
        refused(lib.sa_sum_f64(ptrs(A, B), k, 0, OUT, None), "sa_sum_f64: bad arguments")
    refused(lib.sa_sum_f64(ptrs(None, B), 2, 64, OUT, None), "sa_sum_f64: input 0 null")
    refused(lib.sa_sum_f64(ptrs(A, B, None), 3, 64, OUT, None), "sa_sum_f64: input 2 null")
    refused(lib.sa_sum_f64(ptrs(0x1008, None), 2, 64, 0x1008, None), "sa_sum_f64: input 1 null")
    for n in SERVER_TOO_MANY:  # 16-byte aligned operands take the tile grid
        refused(lib.sa_sum_f64(ptrs(A, B), 2, n, OUT, None), server_launch(n))
        refused(lib.sa_sum_f64(ptrs(A), 1, n, A, None), server_launch(n))
        refused(lib.sa_sum_f64(ptrs(A, None), 2, n, OUT, None), "sa_sum_f64: input 1 null")
    assert lib.sa_sum_f64(None, 1, 0, None, None) == L.SA_OK
    assert lib.sa_sum_f64(ptrs(0x1001), 3, 0, 0x1001, None) == L.SA_OK


# ---------------------------------------------------------------------------
# sa_sumsq_f32, sa_dp_perturb_f32, sa_mask_dp
# ---------------------------------------------------------------------------
def dp(sumsq=SUMSQ, layer=None, updates=4.0, counter0=0):
    return C.byref(L.DP(sumsq, layer, 1.0, 0.5, updates, 7, counter0))


def bad_dps(make):
    """Every way the fields sa_dp and sa_dp_secure share can be refused."""
    yield None
    yield make(sumsq=None)
    yield make(sumsq=None, layer=A)
    for updates in (0.0, -0.0, -1.0, float("nan"), float("-inf")):
        yield make(updates=updates)
    for counter0 in (1, 2, 3, 5, 4 * 2**40 + 2, 2**64 - 1):
        yield make(counter0=counter0)
    yield make(sumsq=None, updates=0.0, counter0=1)


def test_sumsq_f32():
    lib = L.lib()
    text = "sa_sumsq_f32: bad arguments (x must be 16-byte aligned)"
    refused(lib.sa_sumsq_f32(None, 64, PART, SUMSQ, 0, None), text)
    refused(lib.sa_sumsq_f32(A, 64, None, SUMSQ, 0, None), text)
    refused(lib.sa_sumsq_f32(A, 64, PART, None, 1, None), text)
    refused(lib.sa_sumsq_f32(None, 0, None, SUMSQ, 0, None), text)  # partials and sumsq even for n == 0
    refused(lib.sa_sumsq_f32(None, 0, PART, None, 0, None), text)
    for bad in MISALIGNED:
        refused(lib.sa_sumsq_f32(bad, 64, PART, SUMSQ, 0, None), text)
        refused(lib.sa_sumsq_f32(bad, 0, PART, SUMSQ, 1, None), text)


def test_dp_perturb_f32():
    lib = L.lib()
    args = "sa_dp_perturb_f32: bad arguments (16-byte aligned x and out required)"
    bad_dp = "sa_dp_perturb_f32: bad sa_dp (sumsq set, num_updates > 0, counter0 % 4 == 0 required)"
    refused(lib.sa_dp_perturb_f32(None, 64, dp(), OUT, None), args)
    refused(lib.sa_dp_perturb_f32(A, 64, dp(), None, None), args)
    for bad in MISALIGNED:
        refused(lib.sa_dp_perturb_f32(bad, 64, dp(), OUT, None), args)
        refused(lib.sa_dp_perturb_f32(A, 64, dp(), bad, None), args)
        refused(lib.sa_dp_perturb_f32(bad, 0, dp(), None, None), args)  # alignment even of nothing
        refused(lib.sa_dp_perturb_f32(None, 0, dp(), bad, None), args)
    refused(lib.sa_dp_perturb_f32(None, 64, None, OUT, None), args)  # the operands first
    for d in bad_dps(dp):
        refused(lib.sa_dp_perturb_f32(A, 64, d, OUT, None), bad_dp)
        refused(lib.sa_dp_perturb_f32(A, 64, d, A, None), bad_dp)  # in place
        refused(lib.sa_dp_perturb_f32(None, 0, d, None, None), bad_dp)  # even of nothing
        refused(lib.sa_dp_perturb_f32(A, 2**41, d, OUT, None), bad_dp)  # before the size
    for n in DP_TOO_MANY:
        refused(lib.sa_dp_perturb_f32(A, n, dp(), OUT, None), "sa_dp_perturb_f32: n too large for the tile grid")
        refused(lib.sa_dp_perturb_f32(A, n, dp(layer=B, updates=3.0, counter0=2**63), A, None),
                "sa_dp_perturb_f32: n too large for the tile grid")
    assert lib.sa_dp_perturb_f32(None, 0, dp(), None, None) == L.SA_OK
    assert lib.sa_dp_perturb_f32(A, 0, dp(layer=B, counter0=8), OUT, None) == L.SA_OK


def test_mask_dp_own_checks():
    lib = L.lib()
    streams = (L.MaskStream * 1)()

    def mask_dp(x, n, d):
        return lib.sa_mask_dp(x, n, 1.0, 18, streams, 1, d, OUT, None, None, None, None)

    refused(mask_dp(None, 64, dp()), "sa_mask_dp: x is required")
    refused(mask_dp(None, 64, None), "sa_mask_dp: x is required")  # x first
    bad_dp = "sa_mask_dp: bad sa_dp (sumsq set, num_updates > 0, counter0 % 4 == 0 required)"
    for d in bad_dps(dp):
        refused(mask_dp(A, 64, d), bad_dp)
        refused(mask_dp(None, 0, d), bad_dp)  # even of nothing


# ---------------------------------------------------------------------------
# sa_dp_perturb_secure_f32, sa_chacha20_keystream, sa_hb_normals_f64
# ---------------------------------------------------------------------------
def dp_secure(sumsq=SUMSQ, layer=None, updates=4.0, counter0=0):
    return C.byref(L.DPSecure(sumsq, layer, 1.0, 0.5, updates, L.chacha_key_words(bytes(range(32))), 9, counter0))


def test_dp_perturb_secure_f32():
    lib = L.lib()
    args = "sa_dp_perturb_secure_f32: bad arguments (16-byte aligned x and out required)"
    bad_dp = ("sa_dp_perturb_secure_f32: bad sa_dp_secure (sumsq set, num_updates > 0, counter0 % 4 == 0 "
              "required)")
    grid = "sa_dp_perturb_secure_f32: too many elements for the tile grid"
    refused(lib.sa_dp_perturb_secure_f32(None, 64, dp_secure(), OUT, None), args)
    refused(lib.sa_dp_perturb_secure_f32(A, 64, dp_secure(), None, None), args)
    for bad in MISALIGNED:
        refused(lib.sa_dp_perturb_secure_f32(bad, 64, dp_secure(), OUT, None), args)
        refused(lib.sa_dp_perturb_secure_f32(A, 64, dp_secure(), bad, None), args)
        refused(lib.sa_dp_perturb_secure_f32(bad, 0, dp_secure(), None, None), args)  # alignment even of nothing
        refused(lib.sa_dp_perturb_secure_f32(None, 0, dp_secure(), bad, None), args)
    refused(lib.sa_dp_perturb_secure_f32(None, 64, None, OUT, None), args)  # the operands first
    for d in bad_dps(dp_secure):
        refused(lib.sa_dp_perturb_secure_f32(A, 64, d, OUT, None), bad_dp)
        refused(lib.sa_dp_perturb_secure_f32(A, 64, d, A, None), bad_dp)  # in place
        refused(lib.sa_dp_perturb_secure_f32(None, 0, d, None, None), bad_dp)  # even of nothing
        refused(lib.sa_dp_perturb_secure_f32(A, 2**41, d, OUT, None), bad_dp)  # before the size
    for n in DP_TOO_MANY:
        refused(lib.sa_dp_perturb_secure_f32(A, n, dp_secure(), OUT, None), grid)
        refused(lib.sa_dp_perturb_secure_f32(A, n, dp_secure(layer=B, updates=3.0, counter0=2**63), A, None), grid)
    assert lib.sa_dp_perturb_secure_f32(None, 0, dp_secure(), None, None) == L.SA_OK
    assert lib.sa_dp_perturb_secure_f32(A, 0, dp_secure(layer=B, counter0=8), OUT, None) == L.SA_OK


def test_chacha20_keystream():
    lib = L.lib()
    key = L.chacha_key_words(bytes(range(32)))
    text = "sa_chacha20_keystream: bad arguments (key and a 16-byte aligned out required)"
    refused(lib.sa_chacha20_keystream(None, 1, 0, 4, OUT, None), text)
    refused(lib.sa_chacha20_keystream(None, 1, 0, 0, OUT, None), text)  # the key even for no blocks
    refused(lib.sa_chacha20_keystream(key, 1, 0, 4, None, None), text)
    for bad in MISALIGNED:
        refused(lib.sa_chacha20_keystream(key, 1, 0, 4, bad, None), text)
        refused(lib.sa_chacha20_keystream(key, 1, 0, 0, bad, None), text)
    for n in LANES_TOO_MANY:
        refused(lib.sa_chacha20_keystream(key, 1, 0, n, OUT, None),
                "sa_chacha20_keystream: too many elements for the tile grid")
        refused(lib.sa_chacha20_keystream(key, 2**64 - 1, 2**64 - 1, n, OUT, None),
                "sa_chacha20_keystream: too many elements for the tile grid")
        refused(lib.sa_chacha20_keystream(key, 1, 0, n, None, None), text)  # the operands first
    assert lib.sa_chacha20_keystream(key, 1, 0, 0, None, None) == L.SA_OK
    assert lib.sa_chacha20_keystream(key, 1, 2**63, 0, OUT, None) == L.SA_OK


def test_hb_normals_f64():
    lib = L.lib()
    text = "sa_hb_normals_f64: bad arguments (words and out required)"
    refused(lib.sa_hb_normals_f64(None, 4, 1.0, OUT, None), text)
    refused(lib.sa_hb_normals_f64(A, 4, 1.0, None, None), text)
    refused(lib.sa_hb_normals_f64(None, 1, 1.0, None, None), text)
    for n in LANES_TOO_MANY:
        refused(lib.sa_hb_normals_f64(A, n, 1.0, OUT, None), "sa_hb_normals_f64: too many elements for the tile grid")
        refused(lib.sa_hb_normals_f64(0x1004, n, 0.0, 0x1008, None),
                "sa_hb_normals_f64: too many elements for the tile grid")  # element alignment is enough
        refused(lib.sa_hb_normals_f64(None, n, 1.0, OUT, None), text)  # the operands first
    assert lib.sa_hb_normals_f64(None, 0, 1.0, None, None) == L.SA_OK
    assert lib.sa_hb_normals_f64(A, 0, 0.0, OUT, None) == L.SA_OK
