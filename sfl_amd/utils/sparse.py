"""COO transport of compressed updates: the counterpart of the reference's
``sparse_encode`` / ``sparse_decode`` (``sfl/utils/compressor/
sparse_compressor.py:234-284``), which wrap ``sparse.COO``.

A tensor travels as ``SparseCOO``: its shape and dtype, ``index`` (the flat
C-order positions of its non-zeros, ``int32``, strictly ascending) and
``data`` (their values, bit for bit).  **"Non-zero" is decided on the bit
pattern**, ``(bits & ~sign) != 0``: NaN, inf and every denormal are kept,
``+0.0`` and ``-0.0`` are dropped, and a dropped ``-0.0`` decodes as ``+0.0``.

This is the host form: numpy arrays and CPU tensors, of any element type
(integer entries of a state dict, ``num_batches_tracked``, included), run
numpy.  There is no device kernel for it yet, and a CUDA tensor is refused
with ``NotImplementedError`` rather than carried across the host quietly: a
GPU worker that wants sparse transport compresses on its GPU and uploads from
the host (``FedSTC`` with a host model and a GPU ``compress_device``).  A
payload is another party's data: decoding validates every entry (inside the
tensor, strictly ascending, hence unique) and raises ``ValueError`` naming
the tensor.
"""

from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

_UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
_MAX_N = 1 << 31


def _np_dtype(dtype) -> np.dtype:
    if isinstance(dtype, torch.dtype):
        return np.dtype(str(dtype).replace("torch.", "").replace("bool", "bool_"))
    return np.dtype(dtype)


def _size(shape) -> int:
    n = 1
    for d in shape:
        n *= int(d)
    return n


def nonzero_mask(flat: np.ndarray) -> np.ndarray:
    """The bit rule on a flat host array: everything but the sign bit, for
    floats; ``!= 0`` for integers and bools."""
    if flat.dtype.kind == "f":
        u = _UINT[flat.dtype.itemsize]
        return (flat.view(u) << u(1)) != 0
    return flat != 0


class SparseCOO:
    """One tensor in COO form.  ``index`` and ``data`` are two numpy arrays,
    or two CPU tensors; ``dtype`` is the dense tensor's element
    type as a numpy dtype."""

    __slots__ = ("shape", "dtype", "index", "data")

    def __init__(self, shape, dtype, index, data):
        self.shape = tuple(int(d) for d in shape)
        self.dtype = _np_dtype(dtype)
        self.index = index
        self.data = data

    @property
    def size(self) -> int:
        return _size(self.shape)

    @property
    def nnz(self) -> int:
        return int(self.data.numel() if isinstance(self.data, torch.Tensor) else self.data.size)

    @property
    def nbytes(self) -> int:
        """Index plus data: what travels."""
        return self.nnz * (4 + self.dtype.itemsize)

    @property
    def coords(self) -> np.ndarray:
        """The ``(ndim, nnz)`` int64 coordinates, as ``sparse.COO.coords``."""
        idx = _host(self.index).astype(np.int64)
        if not self.shape:
            return np.zeros((0, idx.size), dtype=np.int64)
        return np.stack(np.unravel_index(idx, self.shape)).astype(np.int64).reshape(len(self.shape), idx.size)

    def todense(self):
        return _decode_one(self, "SparseCOO")

    def to(self, device) -> "SparseCOO":
        """Index and data on ``device`` (a torch device).  Only the CPU holds a
        ``SparseCOO`` in this build: there they are numpy arrays."""
        if torch.device(device).type != "cpu":
            raise _no_kernel("SparseCOO.to")
        return SparseCOO(self.shape, self.dtype, _host(self.index), _host(self.data))

    def __repr__(self):
        where = str(self.data.device) if isinstance(self.data, torch.Tensor) else "host"
        return f"SparseCOO(shape={self.shape}, dtype={self.dtype}, nnz={self.nnz}, {where})"


def _no_kernel(what: str) -> NotImplementedError:
    return NotImplementedError(f"{what}: there is no device kernel for the COO form in this build; "
                               f"encode and decode host arrays (CPU tensors, numpy)")


def _host(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        if a.is_cuda:
            raise _no_kernel("SparseCOO")
        return a.detach().numpy()
    return np.asarray(a)


# ---------------------------------------------------------------------------
# encode
# ---------------------------------------------------------------------------
def _encode_host(x: np.ndarray) -> SparseCOO:
    flat = np.ascontiguousarray(x).reshape(-1)
    if flat.size >= _MAX_N:
        raise ValueError("sparse_encode: a tensor of 2^31 elements or more has no int32 flat index")
    idx = np.flatnonzero(nonzero_mask(flat))
    return SparseCOO(x.shape, x.dtype, idx.astype(np.int32), flat[idx])


def _encode_one(x):
    if isinstance(x, SparseCOO):
        return x
    if isinstance(x, torch.Tensor):
        if x.is_cuda:
            raise _no_kernel("sparse_encode")
        c = _encode_host(x.detach().numpy())  # a CPU tensor stays one: two CPU tensors
        return SparseCOO(c.shape, c.dtype, torch.from_numpy(c.index), torch.from_numpy(c.data))
    return _encode_host(np.asarray(x))


def sparse_encode(data: List, encode_method: str = "coo") -> List:
    """The reference's ``sparse_encode``: every entry of ``data`` as a
    ``SparseCOO`` (``None`` gives ``None``)."""
    if data is None:
        return None
    assert encode_method in ["coo", "gcxs"], f"Get unsupport sparse encoding method: {encode_method}, "
    if encode_method == "gcxs":
        raise NotImplementedError("sparse_encode: GCXS is not implemented; use 'coo'")
    return [_encode_one(x) for x in data]


# ---------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------
def _invalid(name: str, why: str) -> ValueError:
    return ValueError(f"sparse payload {name}: {why}")


def check_host_payload(index: np.ndarray, n: int, name: str) -> None:
    """Every entry inside the tensor and above its predecessor."""
    if index.size == 0:
        return
    idx = index.astype(np.int64)
    if np.any(idx < 0) or np.any(idx >= n):
        raise _invalid(name, f"an index lies outside the tensor's {n} elements")
    if np.any(idx[1:] <= idx[:-1]):
        raise _invalid(name, "the indices are not strictly ascending (unsorted or duplicated)")


def _check_form(c: SparseCOO, name: str):
    index, data = c.index, c.data
    if isinstance(index, torch.Tensor) != isinstance(data, torch.Tensor):
        raise _invalid(name, "index and data are two numpy arrays or two tensors")
    if isinstance(index, torch.Tensor):
        if index.device != data.device or index.dtype != torch.int32 or index.dim() != 1 or data.dim() != 1:
            raise _invalid(name, "index is a flat int32 tensor on the data's device")
        if _np_dtype(data.dtype) != c.dtype:
            raise _invalid(name, f"data is {data.dtype}, the tensor {c.dtype}")
    else:
        if index.dtype != np.int32 or index.ndim != 1 or data.ndim != 1:
            raise _invalid(name, "index is a flat int32 array")
        if data.dtype != c.dtype:
            raise _invalid(name, f"data is {data.dtype}, the tensor {c.dtype}")
    if c.nnz != int(index.numel() if isinstance(index, torch.Tensor) else index.size):
        raise _invalid(name, "index and data differ in length")
    if c.size >= _MAX_N:
        raise _invalid(name, "a tensor of 2^31 elements or more has no int32 flat index")
    if c.nnz > c.size:
        raise _invalid(name, "more entries than the tensor has elements")


def _decode_one(c: SparseCOO, name: str):
    _check_form(c, name)
    index, data = _host(c.index), _host(c.data)
    check_host_payload(index, c.size, name)
    dense = np.zeros(c.size, dtype=c.dtype)
    dense[index] = data
    dense = dense.reshape(c.shape)
    return torch.from_numpy(dense) if isinstance(c.data, torch.Tensor) else dense


def _from_foreign(x, name: str) -> SparseCOO:
    """An object with ``coords``, ``data`` and ``shape`` (``sparse.COO``)."""
    shape = tuple(int(d) for d in x.shape)
    coords, data = np.asarray(x.coords), np.asarray(x.data)
    if coords.ndim != 2 or coords.shape[0] != len(shape) or coords.shape[1] != data.size:
        raise _invalid(name, "coords is (ndim, nnz)")
    if _size(shape) >= _MAX_N:
        raise _invalid(name, "a tensor of 2^31 elements or more has no int32 flat index")
    for axis, d in enumerate(shape):
        if coords.shape[1] and (coords[axis].min() < 0 or coords[axis].max() >= d):
            raise _invalid(name, "an index lies outside the tensor")
    flat = np.ravel_multi_index(tuple(coords), shape).astype(np.int64) if shape else np.zeros(data.size, np.int64)
    order = np.argsort(flat, kind="stable")  # sparse.COO keeps C order already; be sure
    return SparseCOO(shape, data.dtype, flat[order].astype(np.int32), data.reshape(-1)[order])


def as_coo(x, name: str = "entry") -> Optional[SparseCOO]:
    """``x`` as a ``SparseCOO`` if it is a sparse entry, else None."""
    if isinstance(x, SparseCOO):
        return x
    if not isinstance(x, (np.ndarray, torch.Tensor)) and all(hasattr(x, a) for a in ("coords", "data", "shape")):
        return _from_foreign(x, name)
    return None


def sparse_decode(data: List) -> List:
    """The reference's ``sparse_decode``: the dense tensors of a list of
    ``SparseCOO``s (or of objects with ``coords``, ``data`` and ``shape``).
    numpy payloads give numpy arrays, CPU-tensor payloads CPU tensors.  An
    invalid payload raises ``ValueError``."""
    if data is None:
        return None
    out = []
    for i, x in enumerate(data):
        c = as_coo(x, f"[{i}]")
        assert c is not None, "Sparse encoding method not supporterd, Only COO GCXS supported"
        out.append(_decode_one(c, f"[{i}]"))
    return out


def payload_nbytes(payload) -> int:
    """Bytes of a list of dense arrays, tensors, ``SparseCOO``s, or a mix."""
    if payload is None:
        return 0
    if isinstance(payload, (list, tuple)):
        return sum(payload_nbytes(p) for p in payload)
    if isinstance(payload, SparseCOO):
        return payload.nbytes
    if isinstance(payload, torch.Tensor):
        return payload.numel() * payload.element_size()
    c = as_coo(payload)
    return c.nbytes if c is not None else int(np.asarray(payload).nbytes)
