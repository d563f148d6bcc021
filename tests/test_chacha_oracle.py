"""The numpy restatement of the secure DP noise (tests/chacha_oracle.py)
against known answers -- RFC 8439's block and openssl's bytes
(tests/golden/chacha20_kat.json) -- and the statistics of its normals, each
within its formula bound (tests/dp_noise_stats.py)."""
import json
import os

import numpy as np
import pytest

import chacha_oracle as co
import dp_noise_stats as S

KEY_A, KEY_B, NONCE = bytes(range(32)), bytes(range(1, 33)), 7


@pytest.fixture(scope="module")
def kat(golden_dir):
    with open(os.path.join(golden_dir, "chacha20_kat.json")) as f:
        return [(e["source"], bytes.fromhex(e["key"]), int(e["nonce"], 16), int(e["block"], 16),
                 np.array([int(w, 16) for w in e["words"]], dtype=np.uint32)) for e in json.load(f)]


def test_restatement_equals_the_known_answers(kat):
    assert kat[0][0].startswith("RFC 8439") and kat[0][3] == 0x0900000000000001 and kat[0][4][0] == 0xE4E7F110
    assert len(kat) >= 8
    for source, key, nonce, block, words in kat:
        got = co.blocks(co.key_words(key), nonce, block, 1)
        assert got.shape == (1, 16) and got.dtype == np.uint32
        assert np.array_equal(got[0], words), (source, hex(block))


def test_block_counter_carries_into_word_13(kat):
    """Golden blocks (word 13 = h, word 12 = 2^32 - 1) and (h + 1, 0), each
    from an openssl call of its own, are consecutive blocks of the 64-bit
    counter; the counter wraps mod 2^64."""
    by = {(key, nonce, block): words for _, key, nonce, block, words in kat}
    pairs = [(k, n, b) for (k, n, b) in by if b & 0xFFFFFFFF == 0xFFFFFFFF and (k, n, (b + 1) & co.M64) in by]
    assert len(pairs) >= 3 and (KEY_A, NONCE, (1 << 64) - 1) in pairs
    for key, nonce, b in pairs:
        got = co.blocks(co.key_words(key), nonce, b, 2)
        assert np.array_equal(got[0], by[(key, nonce, b)]), hex(b)
        assert np.array_equal(got[1], by[(key, nonce, (b + 1) & co.M64)]), hex(b)


def test_uniforms_and_the_transform_at_hand_computed_points():
    """u = the top 53 bits of the word pair over 2^53; u2 = 0 gives r = 0;
    u1 = 1/8 gives sin = cos: z = r sigma, up to the rounding of sin(pi/4)."""
    w = np.array([[0xFFFFFFFF, 0xFFFFFFFF, 0, 0], [0x7FF, 0, 0x800, 0], [0, 0x20000000, 0, 0x80000000]],
                 dtype=np.uint32)
    u1, u2 = co.uniforms(w)
    assert u1.tolist() == [1 - 2.0**-53, 0.0, 0.125] and u2.tolist() == [0.0, 2.0**-53, 0.5]
    z = co.normals_of_words(w, 3.0)
    assert z[0] == 0.0
    assert abs(z[2] - 3.0 * np.sqrt(2.0 * np.log(2.0))) < 1e-14
    assert np.array_equal(co.normals64(co.key_words(KEY_A), NONCE, 8, 5, 1.0),
                          co.normals64(co.key_words(KEY_A), NONCE, 0, 16, 1.0)[8:13])


def test_noise_statistics_of_the_restatement():
    """2^22 normals of KEY_A, of KEY_B at the same counters and of KEY_A's
    next window: moments, CDF, tails, autocorrelations and the two
    correlations inside their formula bounds."""
    z, zk, zn = (co.normals64(co.key_words(k), NONCE, c, S.N, 1.0) for k, c in ((KEY_A, 0), (KEY_B, 0), (KEY_A, S.N)))
    assert np.all(np.isfinite(z)) and not np.array_equal(z, zk) and not np.array_equal(z, zn)
    S.check_noise_statistics(S.noise_statistics(z, zk, zn), "restatement")
