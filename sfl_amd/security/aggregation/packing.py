"""pack=2 on the host: two 32-bit fixed-point values per 64-bit ring word.

The numpy form of what ``sa_mask_pack2`` / ``sa_fused_clients_pack2`` build
and ``sa_decode_pack2`` undoes (include/sfl_sa.h): the masks,
the ring Z/2^64 and the server's sum are the unpacked protocol's; only the
quantized vector is packed before masking and unpacked after the sum.
"""

from __future__ import annotations

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def pack_limit(n_clients: int) -> np.float32:
    """The range rule's bound on ``|x * w * 2^fxp|``: the largest float32
    not above ``2^31 / n_clients`` (products must stay strictly below it)."""
    d = 2.0 ** 31 / n_clients
    f = np.float32(d)
    return f if float(f) <= d else np.nextafter(f, np.float32(0))


def pack_words(q, n_clients: int = 1) -> np.ndarray:
    """The ``ceil(n / 2)`` ring words (uint64) of ``n`` quantized values:
    ``W[j] = sext64(q[2j]) + (sext64(q[2j+1]) << 32) mod 2^64``, ``q[n] = 0``
    for odd ``n``.  Raises ``OverflowError`` unless every ``|q| * n_clients <
    2^31``: the sum of ``n_clients`` such vectors then fits 32 bits per value."""
    q = np.asarray(q, dtype=np.int64).reshape(-1)
    if q.size and int(np.abs(q).max()) * int(n_clients) >= 1 << 31:
        raise OverflowError(f"pack=2: |q| must stay below 2^31 / {n_clients} (got {int(np.abs(q).max())})")
    if q.size & 1:
        q = np.append(q, np.int64(0))
    u = q.view(np.uint64)
    return u[0::2] + (u[1::2] << np.uint64(32))


def unpack_words(S, n: int) -> np.ndarray:
    """The ``n`` int64 sums in the summed words ``S``: ``lo = int32(S)``,
    ``hi = int32((S >> 32) + (lo < 0))`` -- the borrow that the low halves'
    sign extension took from the high half."""
    S = np.asarray(S, dtype=np.uint64).reshape(-1)
    lo = (S & _M32).astype(np.uint32).view(np.int32)
    hi = (((S >> np.uint64(32)) + (lo < 0)) & _M32).astype(np.uint32).view(np.int32)
    out = np.empty(2 * S.size, dtype=np.int64)
    out[0::2], out[1::2] = lo, hi
    return out[:n]
