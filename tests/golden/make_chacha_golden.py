"""Regenerates tests/golden/chacha20_kat.json: known answers for the
ChaCha20 keystream of include/sfl_sa.h (state words 12, 13: a 64-bit block
counter; 14, 15: a 64-bit nonce).

    python tests/golden/make_chacha_golden.py

* the block of RFC 8439 section 2.3.2 (typed in from the RFC; in this
  layout: block 0x0900000000000001, nonce 0x4a000000), which the local
  openssl must reproduce;
* blocks from ``openssl enc -chacha20`` over 64 zero bytes, its 16-byte IV
  being the state words 12..15, little-endian.  Every block is one openssl
  call of its own with all four words given, so openssl's own counter carry
  is never relied on: the pairs (word 13 = h, word 12 = 2^32 - 1) and
  (word 13 = h + 1, word 12 = 0) are consecutive blocks of the 64-bit counter
  and pin its carry.

Data only: key, nonce, block number and the block's 16 words, in hex.
"""
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
KEY_A = bytes(range(32))
KEY_B = bytes(range(1, 33))

RFC_WORDS = """e4e7f110 15593bd1 1fdd0f50 c47120a3 c7f4d1c7 0368c033 9aaa2204 4e6cd4c3
               466482d2 09aa9f07 05d7c214 a2028bd9 d19c12b5 b94e16de e883d0cb 4e3c50a2""".split()

CASES = [  # (key, nonce, block)
    (KEY_A, 7, 0),
    (KEY_A, 7, 1),
    (KEY_B, 7, 0),
    (KEY_A, (1 << 63) + 9, 3),
    (KEY_A, 7, (1 << 32) - 1),          # word 13 = 0, word 12 = 2^32 - 1
    (KEY_A, 7, 1 << 32),                # word 13 = 1, word 12 = 0: the next block
    (KEY_B, 7, (0x100 << 32) + 0xFFFFFFFF),  # h = 0x100
    (KEY_B, 7, 0x101 << 32),                 # h + 1
    (KEY_A, 7, (1 << 40) + 5),
    (KEY_A, 7, (1 << 64) - 1),
]


def openssl_block(key: bytes, nonce: int, block: int) -> list:
    iv = block.to_bytes(8, "little") + nonce.to_bytes(8, "little")
    out = subprocess.run(["openssl", "enc", "-chacha20", "-K", key.hex(), "-iv", iv.hex()], input=bytes(64),
                         capture_output=True, check=True).stdout
    assert len(out) == 64, len(out)
    return [f"{int.from_bytes(out[4 * i:4 * i + 4], 'little'):08x}" for i in range(16)]


def entry(source, key, nonce, block, words):
    return {"source": source, "key": key.hex(), "nonce": f"{nonce:#x}", "block": f"{block:#x}", "words": words}


def main():
    rfc = (KEY_A, 0x4A000000, 0x0900000000000001)
    assert openssl_block(*rfc) == RFC_WORDS, "openssl disagrees with RFC 8439 2.3.2"
    out = [entry("RFC 8439 2.3.2", *rfc, RFC_WORDS)]
    out += [entry("openssl enc -chacha20", k, n, b, openssl_block(k, n, b)) for k, n, b in CASES]
    with open(os.path.join(HERE, "chacha20_kat.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"{len(out)} blocks")


if __name__ == "__main__":
    main()
