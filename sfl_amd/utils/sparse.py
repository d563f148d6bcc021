"""COO transport of compressed updates: the counterpart of the reference's
``sparse_encode`` / ``sparse_decode`` (``sfl/utils/compressor/
sparse_compressor.py:234-284``), which wrap ``sparse.COO``.

A tensor travels as ``SparseCOO``: its shape and dtype, ``index`` (the flat
C-order positions of its non-zeros, ``int32``, strictly ascending) and
``data`` (their values, bit for bit).  **"Non-zero" is decided on the bit
pattern**, ``(bits & ~sign) != 0``: NaN, inf and every denormal are kept,
``+0.0`` and ``-0.0`` are dropped, and a dropped ``-0.0`` decodes as ``+0.0``.

There are two forms.  The host form: numpy arrays and CPU tensors, of any
element type (integer entries of a state dict, ``num_batches_tracked``,
included), run numpy.  The device form: a CUDA float32 / float64 tensor is
encoded and decoded where it lives by the ``sa_coo_*`` kernels
(``sfl_amd/csrc/sa_coo.hip``: count, one pinned read of ``nnz``, fill; a
validated scatter), and ``index`` and ``data`` are tensors on that device.  A
CUDA tensor of any other element type is a counter of a few elements: it comes
to the host through pinned memory and takes the host form.  A payload is
another party's data: decoding validates every entry (inside the tensor,
strictly ascending, hence unique) and raises ``ValueError`` naming the tensor,
with the same words in both forms.
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
    or two tensors on one device (the CPU or a GPU); ``dtype`` is the dense
    tensor's element type as a numpy dtype."""

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
        """Index and data on ``device`` (a torch device): numpy arrays on the
        CPU, tensors on a GPU.  Host and device exchange them through pinned
        memory (``hostpipe.h2d`` / ``d2h``)."""
        device = torch.device(device)
        if device.type == "cpu":
            return SparseCOO(self.shape, self.dtype, _host(self.index), _host(self.data))
        from .. import hostpipe as H

        return SparseCOO(self.shape, self.dtype, H.h2d(self.index, device), H.h2d(self.data, device))

    @property
    def is_device(self) -> bool:
        return isinstance(self.data, torch.Tensor) and self.data.is_cuda

    def __repr__(self):
        where = str(self.data.device) if isinstance(self.data, torch.Tensor) else "host"
        return f"SparseCOO(shape={self.shape}, dtype={self.dtype}, nnz={self.nnz}, {where})"


def _host(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        if a.is_cuda:
            from .. import hostpipe as H

            if a.numel() == 0:
                return np.empty(tuple(a.shape), dtype=H.host_dtype(a))
            return H.d2h(a, pooled=False)  # pinned, never a pageable DMA
        return a.detach().numpy()
    return np.asarray(a)


_DEVICE_FLOATS = (torch.float32, torch.float64)


def _read_words(t: torch.Tensor) -> np.ndarray:
    """A few device words on the host through a pinned buffer (blocking)."""
    from .. import hostpipe as H

    return H.d2h(t, pooled=False)


# ---------------------------------------------------------------------------
# encode
# ---------------------------------------------------------------------------
def _encode_host(x: np.ndarray) -> SparseCOO:
    flat = np.ascontiguousarray(x).reshape(-1)
    if flat.size >= _MAX_N:
        raise ValueError("sparse_encode: a tensor of 2^31 elements or more has no int32 flat index")
    idx = np.flatnonzero(nonzero_mask(flat))
    return SparseCOO(x.shape, x.dtype, idx.astype(np.int32), flat[idx])


def _encode_device(x: torch.Tensor) -> SparseCOO:
    """count, one pinned read of nnz, allocation, fill: index and data on x's device."""
    from .. import kernels as K

    flat = x.detach().contiguous().reshape(-1)
    n, dev = flat.numel(), flat.device
    if n >= _MAX_N:
        raise ValueError("sparse_encode: a tensor of 2^31 elements or more has no int32 flat index")
    nnz = 0
    if n:
        scratch = torch.empty(K.coo_scratch_bytes(n, flat.dtype) // 4, dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        K.coo_count(flat, scratch, count)
        nnz = int(_read_words(count)[0])
    index = torch.empty(nnz, dtype=torch.int32, device=dev)
    data = torch.empty(nnz, dtype=flat.dtype, device=dev)
    if nnz:
        # x has not changed since the count (one stream), so the count holds and the flag is
        # not read; were it to differ, no entry beyond nnz would be stored
        K.coo_fill(flat, scratch, index, data, K.coo_flag(dev))
    return SparseCOO(x.shape, x.dtype, index, data)


def _encode_one(x):
    if isinstance(x, SparseCOO):
        return x
    if isinstance(x, torch.Tensor):
        if x.is_cuda:
            if x.dtype in _DEVICE_FLOATS:
                return _encode_device(x)
            return _encode_host(_host(x))  # a counter of a few elements: the host form
        c = _encode_host(x.detach().numpy())  # a CPU tensor stays one: two CPU tensors
        return SparseCOO(c.shape, c.dtype, torch.from_numpy(c.index), torch.from_numpy(c.data))
    return _encode_host(np.asarray(x))


def sparse_encode(data: List, encode_method: str = "coo") -> List:
    """The reference's ``sparse_encode``: every entry of ``data`` as a
    ``SparseCOO`` (``None`` gives ``None``).  A host array gives the host form
    and a CPU tensor two CPU tensors.  A CUDA float32 / float64 tensor is
    encoded on its device and gives index and data on that device.  A CUDA
    tensor of any other element type (a state dict's ``num_batches_tracked``)
    is a counter of a few elements: it comes to the host through pinned memory
    (``hostpipe.d2h``) and gives a host ``SparseCOO`` of numpy arrays."""
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


def flag_error(bits: int, n: int, name: str) -> Optional[ValueError]:
    """What a device flag record (``SA_COO_BAD_*``) says, in
    ``check_host_payload``'s words and order; None when nothing is set."""
    from .._lib import SA_COO_BAD_ORDER, SA_COO_BAD_RANGE

    if bits & SA_COO_BAD_RANGE:
        return _invalid(name, f"an index lies outside the tensor's {n} elements")
    if bits & SA_COO_BAD_ORDER:
        return _invalid(name, "the indices are not strictly ascending (unsorted or duplicated)")
    return None


def _decode_device(c: SparseCOO, name: str) -> torch.Tensor:
    from .. import kernels as K

    dev = c.data.device
    if c.data.dtype not in _DEVICE_FLOATS:  # not what sparse_encode makes: decoded on the host
        from .. import hostpipe as H

        return H.h2d(_decode_one(c.to("cpu"), name), dev)
    dense = torch.empty(c.size, dtype=c.data.dtype, device=dev)
    if c.size:
        flag = K.coo_flag(dev)
        K.coo_decode(c.index.contiguous(), c.data.contiguous(), dense, flag)
        err = flag_error(int(_read_words(flag)[0]), c.size, name)
        if err is not None:
            raise err
    return dense.reshape(c.shape)


def _decode_one(c: SparseCOO, name: str):
    _check_form(c, name)
    if c.is_device:
        return _decode_device(c, name)
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
    numpy payloads give numpy arrays, CPU-tensor payloads CPU tensors, device
    payloads tensors on their device.  An invalid payload raises
    ``ValueError``."""
    if data is None:
        return None
    out = []
    for i, x in enumerate(data):
        c = as_coo(x, f"[{i}]")
        assert c is not None, "Sparse encoding method not supporterd, Only COO GCXS supported"
        out.append(_decode_one(c, f"[{i}]"))
    return out


def payload_nbytes(payload) -> int:
    """Bytes of a list of dense arrays, tensors, ``SparseCOO``s, quantized
    objects (``utils/quantized.py``: their codes), or a mix."""
    if payload is None:
        return 0
    if isinstance(payload, (list, tuple)):
        return sum(payload_nbytes(p) for p in payload)
    from .quantized import QuantizedCompressedData

    if isinstance(payload, (SparseCOO, QuantizedCompressedData)):
        return payload.nbytes
    if isinstance(payload, torch.Tensor):
        return payload.numel() * payload.element_size()
    c = as_coo(payload)
    return c.nbytes if c is not None else int(np.asarray(payload).nbytes)
