"""numpy restatement of sparse ternary compression for the STC tests: the
reference's ``STCSparse`` (sparse_compressor.py:142-179) with the error
feedback around it, ties at the threshold broken by index
(``np.argsort(kind="stable")``: the lower index is masked first), keys
ordered by the bit pattern of ``|u|``.  Written for reading, not speed."""
import math

import numpy as np

_UINT = {np.dtype(np.float32): (np.uint32, 0x7FFFFFFF), np.dtype(np.float64): (np.uint64, 0x7FFFFFFFFFFFFFFF)}


def keys(u):
    """|u|'s bit patterns as unsigned integers (numpy's sort order, NaN last)."""
    ut, m = _UINT[u.dtype]
    return np.ascontiguousarray(u).reshape(-1).view(ut) & ut(m)


def mask_count(rate, n):
    return round(rate * n)


def form(a, b=None, r=None):
    """u = (a - b) + r; an absent operand's operation is not performed."""
    u = a
    if b is not None:
        u = np.subtract(u, b)
    if r is not None:
        u = np.add(u, r)
    return u


def keep_mask(u, mask_num):
    """True where an element survives."""
    keep = np.ones(u.size, dtype=bool)
    keep[np.argsort(keys(u), kind="stable")[:mask_num]] = False
    return keep.reshape(u.shape)


def mu_exact(u, mask_num):
    """The survivors' mean |u| from an exactly rounded sum (a python float)."""
    if mask_num == u.size:
        return 0.0
    keep = keep_mask(u, mask_num).reshape(-1)
    return math.fsum(np.abs(u.reshape(-1)[keep]).astype(np.float64).tolist()) / (u.size - mask_num)


def stc(a, b=None, r=None, mask_num=0, acc=None):
    """(sparse, res, mu, acc'): mu = T(float64 sum of the survivors' |u| /
    (n - mask_num)), the sum taken by numpy over the masked array."""
    u = form(a, b, r)
    T = u.dtype.type
    um = np.where(keep_mask(u, mask_num), u, T(0))
    mu = T(0) if mask_num == u.size else T(np.sum(np.abs(um), dtype=np.float64) / (u.size - mask_num))
    with np.errstate(invalid="ignore"):
        sparse = mu * np.sign(um)
        res = np.subtract(u, sparse)
        acc2 = None if acc is None else np.add(acc, sparse)
    return sparse, res, mu, acc2


def threshold_is_unique(u, mask_num):
    """No other element shares the threshold magnitude (the largest masked
    key), or that magnitude is 0: then every sort order masks the same set,
    up to zeros, which change neither the sum nor a sign."""
    if mask_num == 0 or mask_num == u.size:
        return True
    k = np.sort(keys(u))
    t = k[mask_num - 1]
    return bool(t == 0 or np.count_nonzero(k == t) == 1)


def ulp(x, dtype):
    """Spacing of ``dtype`` at |x|."""
    return float(np.spacing(np.abs(np.dtype(dtype).type(x))))
