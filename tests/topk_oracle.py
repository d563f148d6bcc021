"""An independent restatement of TopkSparse / RandomSparse for the tests: the
``k`` largest keys, the position breaking ties (of equal keys the higher
position counts as larger), written as one lexicographic sort."""
import numpy as np

from oracle import dp


def abs_key(flat: np.ndarray) -> np.ndarray:
    """The bit pattern of |x| as an unsigned integer."""
    if flat.dtype == np.float32:
        return flat.view(np.uint32) & np.uint32(0x7FFFFFFF)
    assert flat.dtype == np.float64
    return flat.view(np.uint64) & np.uint64(0x7FFFFFFFFFFFFFFF)


def kept(keys: np.ndarray, k: int) -> np.ndarray:
    """The positions of the ``k`` largest (key, position) pairs, ascending."""
    n = keys.size
    order = np.lexsort((np.arange(n), keys))  # by key, then by position
    return np.sort(order[n - k:]).astype(np.int32)


def topk(x: np.ndarray, k: int):
    """(index, data, dense) of the top-k of ``x``."""
    flat = np.ascontiguousarray(x).reshape(-1)
    return _payload(x, flat, kept(abs_key(flat), k))


def random_keys(seed: int, n: int) -> np.ndarray:
    """Element e: ((w[2e+1] << 32) | w[2e]) >> 1 of the Philox stream under ``seed``."""
    w = dp.philox_words(seed, 0, 2 * n).reshape(-1).astype(np.uint64)[:2 * n]
    return ((w[1::2] << np.uint64(32)) | w[0::2]) >> np.uint64(1)


def random(x: np.ndarray, k: int, seed: int):
    flat = np.ascontiguousarray(x).reshape(-1)
    return _payload(x, flat, kept(random_keys(seed, flat.size), k))


def _payload(x, flat, index):
    dense = np.zeros(flat.size, dtype=flat.dtype)
    dense[index] = flat[index]
    return index, flat[index], dense.reshape(x.shape)


def same_bits(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
