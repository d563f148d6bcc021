"""numpy restatement of the COO transport (sfl_amd/utils/sparse.py and the
sa_coo_* kernels): what is a non-zero, the encoding, the decoding, and the
aggregates over decoded arrays.  Nothing here imports the package."""
import numpy as np

_UINT = {4: np.uint32, 8: np.uint64}


def bits(x):
    """The bit patterns of a float array (other types: the array itself)."""
    x = np.ascontiguousarray(x)
    return x.view(_UINT[x.dtype.itemsize]) if x.dtype.kind == "f" else x


def nonzero_mask(flat):
    """(bits & ~sign) != 0 for floats: NaN, inf and denormals count, +-0 do not."""
    if flat.dtype.kind != "f":
        return flat != 0
    u = _UINT[flat.dtype.itemsize]
    sign = u(1) << u(8 * flat.dtype.itemsize - 1)
    return (flat.view(u) & ~sign) != 0


def encode(x):
    """(index int64 flat C-order ascending, data) of an array."""
    flat = np.ascontiguousarray(x).reshape(-1)
    idx = np.flatnonzero(nonzero_mask(flat))
    return idx, flat[idx]


def coords(x):
    """The (ndim, nnz) int64 coordinates of the non-zeros."""
    x = np.asarray(x)
    idx, _ = encode(x)
    if x.ndim == 0:
        return np.zeros((0, idx.size), dtype=np.int64)
    return np.stack(np.unravel_index(idx, x.shape)).astype(np.int64)


def decode(idx, data, shape, dtype):
    out = np.zeros(int(np.prod(shape, dtype=np.int64)), dtype=dtype)
    out[np.asarray(idx, dtype=np.int64)] = data
    return out.reshape(shape)


def plus_zero(ref):
    """The one permitted difference: a numpy reduction can give -0.0 where
    the zero-initialised accumulator gives +0.0."""
    return ref + 0.0


def same_bits(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    return got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(bits(got), bits(plus_zero(ref)))


def total(arrays, axis=0):
    return np.sum(arrays, axis=axis)


def average(arrays, axis=0, weights=None):
    return np.average(arrays, axis=axis, weights=weights)


def sequential(xs, ws, A, divide=True):
    """((x0*w0 + x1*w1) + ...) / sum(w) with every operation rounded in A:
    what one sa_coo_axpy per party, then sa_coo_finish, computes."""
    A = np.dtype(A)
    acc = np.zeros(xs[0].shape, dtype=A)
    with np.errstate(invalid="ignore", over="ignore"):
        for x, w in zip(xs, ws):
            acc = acc + x.astype(A) * A.type(w)
        if divide:
            acc = acc / np.asarray(ws).sum(dtype=A)
    return acc
