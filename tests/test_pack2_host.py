"""pack=2 on the host: the packed words' sum unpacks to the sum of the
quantized vectors (the borrow of ``unpack_words``), and ``pack_words``
enforces the range rule ``|q| * C < 2^31``."""
import numpy as np
import pytest

from sfl_amd.security.aggregation.packing import pack_limit, pack_words, unpack_words


@pytest.mark.parametrize("C", [2, 8])
@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("plant", ["random", "neg_low", "all_min", "all_max", "mixed"])
def test_round_trip_pins_the_borrow(C, n, plant):
    bound = (2 ** 31 - 1) // C
    rng = np.random.default_rng(C * 100 + n)
    qs = rng.integers(-bound, bound + 1, size=(C, n), dtype=np.int64)
    if plant == "neg_low":  # every low half negative: each takes a borrow from its high half
        qs[:, 0::2] = -np.abs(qs[:, 0::2]) - 1
        qs[:, 0::2] = np.maximum(qs[:, 0::2], -bound)
    elif plant == "all_min":
        qs[:] = -bound
    elif plant == "all_max":
        qs[:] = bound
    elif plant == "mixed":
        qs[::2] = -bound
        qs[1::2, 0::2] = bound
        qs[1::2, 1::2] = -1
    S = np.zeros((n + 1) // 2, dtype=np.uint64)
    for q in qs:
        S += pack_words(q, C)
    assert np.array_equal(unpack_words(S, n), qs.sum(axis=0))


@pytest.mark.parametrize("C", [2, 8])
def test_value_at_the_bound_raises(C):
    at = 2 ** 31 // C
    assert pack_words([0, at - 1, -(at - 1)], C).size == 2
    for q in (at, -at):
        with pytest.raises(OverflowError):
            pack_words([0, 0, q], C)
    assert float(pack_limit(C)) == 2.0 ** 31 / C and float(pack_limit(3)) <= 2.0 ** 31 / 3
