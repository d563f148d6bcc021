"""numpy restatement of the secure DP noise (test helper): the ChaCha20
keystream and the Holohan-Braghin normal of include/sfl_sa.h, written from
its definition and vectorised over blocks.

* ChaCha20: RFC 8439 section 2.3 (quarter round 2.1, block function 2.3),
  state words 12, 13 a 64-bit block counter, 14, 15 a 64-bit nonce; pinned by
  the RFC's vector and by openssl's bytes in tests/golden/chacha20_kat.json.
* The normal: sfl/security/random/distrbutions.py:124-137 (u1, u2 =
  randbits(53) / 2**53; r = sqrt(-2 log(1 - u2)); theta = 2 pi u1;
  (r sin(theta) std + r cos(theta) std) / sqrt(2)), every step float64.
"""
import numpy as np

CONSTANTS = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)
M64 = (1 << 64) - 1


def key_words(key: bytes) -> list:
    assert len(key) == 32
    return [int.from_bytes(key[4 * i:4 * i + 4], "little") for i in range(8)]


def _rotl(x, n):
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def _quarter(s, a, b, c, d):
    s[a] += s[b]; s[d] ^= s[a]; s[d] = _rotl(s[d], 16)  # noqa: E702
    s[c] += s[d]; s[b] ^= s[c]; s[b] = _rotl(s[b], 12)  # noqa: E702
    s[a] += s[b]; s[d] ^= s[a]; s[d] = _rotl(s[d], 8)  # noqa: E702
    s[c] += s[d]; s[b] ^= s[c]; s[b] = _rotl(s[b], 7)  # noqa: E702


def blocks(key8, nonce: int, b0: int, nb: int) -> np.ndarray:
    """Blocks b0 .. b0 + nb - 1 (mod 2^64) of (key8: eight words, nonce) as
    (nb, 16) uint32."""
    blk = np.arange(nb, dtype=np.uint64) + np.uint64(b0 & M64)  # array addition wraps mod 2^64
    full = lambda v: np.full(nb, v & 0xFFFFFFFF, dtype=np.uint32)  # noqa: E731
    init = [full(c) for c in CONSTANTS] + [full(k) for k in key8]
    init += [(blk & np.uint64(0xFFFFFFFF)).astype(np.uint32), (blk >> np.uint64(32)).astype(np.uint32),
             full(nonce), full(nonce >> 32)]
    s = [w.copy() for w in init]
    for _ in range(10):
        _quarter(s, 0, 4, 8, 12)
        _quarter(s, 1, 5, 9, 13)
        _quarter(s, 2, 6, 10, 14)
        _quarter(s, 3, 7, 11, 15)
        _quarter(s, 0, 5, 10, 15)
        _quarter(s, 1, 6, 11, 12)
        _quarter(s, 2, 7, 8, 13)
        _quarter(s, 3, 4, 9, 14)
    return np.stack([a + b for a, b in zip(s, init)], axis=1)


def uniforms(words: np.ndarray):
    """(u1, u2) of an (n, 4) uint32 array of words a, b, c, d: exact float64."""
    w = words.astype(np.uint64)
    sh, eleven = np.uint64(32), np.uint64(11)
    u1 = (((w[:, 1] << sh) | w[:, 0]) >> eleven).astype(np.float64) * 2.0**-53
    u2 = (((w[:, 3] << sh) | w[:, 2]) >> eleven).astype(np.float64) * 2.0**-53
    return u1, u2


def normals_of_words(words: np.ndarray, sigma: float) -> np.ndarray:
    """z64 of an (n, 4) uint32 array of words, in the reference's operation order."""
    u1, u2 = uniforms(words)
    sigma = np.float64(sigma)
    r = np.sqrt(-2.0 * np.log(1.0 - u2))
    theta = (2.0 * np.pi) * u1
    return ((r * np.sin(theta)) * sigma + (r * np.cos(theta)) * sigma) / np.sqrt(2.0)


def normals64(key8, nonce: int, counter0: int, n: int, sigma: float) -> np.ndarray:
    """z64 of noise indices counter0 .. counter0 + n - 1: index i is normal
    i & 3 of block i >> 2."""
    b0, b1 = counter0 // 4, (counter0 + n + 3) // 4
    z = normals_of_words(blocks(key8, nonce, b0, b1 - b0).reshape(-1, 4), sigma)
    off = counter0 - 4 * b0
    return z[off:off + n]
