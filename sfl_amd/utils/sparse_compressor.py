"""Top-k and random sparsification, and their composition with a quantizer:
the counterpart of the reference's ``TopkSparse`` / ``RandomSparse``
(``sfl/utils/compressor/sparse_compressor.py:23-139``), ``MixedCompressor``
(``mixed_compressor.py:23-111``), the two base classes (``base.py``) and the
``get(name, params)`` factory (``__init__.py``).

The definition.  One tensor of ``origin_shape`` holds ``n`` elements of type T
(float32 or float64); it is seen as ``(origin_shape[0], -1)`` when it has more
than two dimensions, and the flat row-major index is the same in both views.
``k = round((1 - sparse_rate) * n)`` (Python's ``round``) entries are **kept**.

``TopkSparse`` keeps the ``k`` elements of largest ``|x|``, ordered by the bit
pattern of ``|x|`` as an unsigned integer (numpy's order, NaN last, so NaN is
kept first).  **Equal keys at the threshold: the lower indices are dropped
first**, so the kept set is the complement of what ``stc_step`` masks at
``mask_num = n - k`` and ``TopkSparse`` and ``STCSparse`` agree on the support.
The reference's ``np.argpartition`` breaks such ties arbitrarily; this rule is
the refinement.

``RandomSparse(sparse_rate, seed=None)`` keeps ``k`` positions drawn uniformly
without replacement.  Element ``e`` gets a 63-bit key from the Philox4x32-10
stream under a 64-bit seed, ``((w[2e+1] << 32) | w[2e]) >> 1`` with element
``e`` in counter block ``e >> 1``, and the ``k`` largest keys are kept under the
rule above.  The reference draws from an unseeded ``default_rng().choice``, so
parity with it is distributional (as for the DP noise).  ``seed=None`` takes 64
bits from ``secrets``; an instance counts its draws and uses ``seed + draws``
(mod 2^64) per tensor, so two tensors never share keys; ``seed`` and ``draws``
are readable.  Host and device use one definition and give the same index set
for the same seed.

The payload, ``SparseCompressedData``: ``index`` (the kept flat positions,
int32, **strictly ascending**) and ``compressed_data`` (the ``k`` values, bit
for bit), with ``shape`` (2-D), ``origin_shape`` and ``sparse_rate`` under the
reference's names.  The reference stores int64 ``row`` and ``col`` in
``argpartition``'s arbitrary order, on which its dense result does not depend;
here ``row`` and ``col`` are derived from ``index`` on demand, where the payload
lives.  Further refinements:

* ``k == 0`` gives an empty payload.  The reference's ``[-0:]`` slice keeps
  everything at ``sparse_rate = 1``, while its ``RandomSparse`` keeps nothing.
* A 1-D tensor is treated as ``(1, n)`` and restored; the reference raises
  ``ValueError`` on it.  A 0-d input is returned as it is, as in the reference.

``compress(data, sparse_mask=mask)`` takes the values of ``data`` at the mask's
positions, zeros included.  ``get_sparse_mask()`` gives a scipy ``csr_matrix``
of bool for a host payload, as the reference does, and a ``SparseMask`` (the
device ``index`` and ``shape``) for a device payload; ``compress`` accepts
either kind where the data lives (a host mask with device data is moved once
through ``hostpipe.h2d``).

``MixedCompressor(sparse, quantized)`` is the reference's composition: the
sparse compressor's ``k`` values, a 1-D vector, go through the quantizer.
``MixedCompressedData.compressed_data`` is the codes; the two participants
carry ``None`` data until ``decompress`` puts it back.  An empty payload
raises ``ValueError``: a range of nothing cannot be quantized.

Where it runs.  CUDA float32 / float64 tensors run the kernels of
``sfl_amd/csrc/sa_topk.hip`` (a radix select, then a ballot-rank compaction;
``k`` is known on the host, so nothing is read back and nothing synchronises)
and give device payloads.  numpy arrays and CPU tensors run numpy (a stable
argsort on the key).  ``decompress`` gives back what went in.  A payload is
another party's data: ``decompress`` validates it like ``sparse_decode`` and
raises ``ValueError`` naming the entry; an index out of range is never used.
"""

from __future__ import annotations

import logging
import secrets
from typing import Dict, List, Union

import numpy as np
import torch

from .quantized import QuantizedCompressedData, QuantizedCompressor
from .sparse import _MAX_N, SparseCOO, _decode_one, _host, _np_dtype, _size, check_host_payload

_KEY = {np.dtype(np.float32): (np.uint32, np.uint32(0x7FFFFFFF)),
        np.dtype(np.float64): (np.uint64, np.uint64(0x7FFFFFFFFFFFFFFF))}
_M64 = (1 << 64) - 1


def keep_count(sparse_rate: float, n: int) -> int:
    """The reference's ``round((1 - self.sparse_rate) * data_len)``."""
    return round((1 - sparse_rate) * n)


def topk_index(flat: np.ndarray, k: int) -> np.ndarray:
    """The kept positions of a flat float32 / float64 host array, ascending."""
    kt, km = _KEY[flat.dtype]
    return largest_keys_index(flat.view(kt) & km, k)


def largest_keys_index(keys: np.ndarray, k: int) -> np.ndarray:
    """The positions of the ``k`` largest unsigned keys, ascending; among equal
    keys at the threshold the higher positions."""
    order = np.argsort(keys, kind="stable")
    return np.sort(order[keys.size - k:]).astype(np.int32)


# ---------------------------------------------------------------------------
# the reference's two bases
# ---------------------------------------------------------------------------
class CompressedData:
    """Data after compression."""

    def __init__(self, compressed_data):
        self.compressed_data = compressed_data


class Compressor:
    """The reference's ``Compressor``: ``compress`` takes an array (numpy, a
    CPU tensor or a CUDA tensor) and gives one compressed object, or a list /
    tuple of arrays and gives a list; ``decompress`` and ``iscompressed`` take
    one object or a list."""

    def compress(self, data, **kwargs):
        if isinstance(data, (np.ndarray, torch.Tensor)):
            return self._compress_one(data, "[0]", **kwargs)
        if not isinstance(data, (list, tuple)):
            raise TypeError(f"invalid data: {type(data)}")
        return [self._compress_one(d, f"[{i}]", **kwargs) for i, d in enumerate(data)]

    def decompress(self, data):
        if not isinstance(data, list):
            return self._decompress_one(data, "[0]")
        return [self._decompress_one(d, f"[{i}]") for i, d in enumerate(data)]

    def iscompressed(self, data):
        if not isinstance(data, list):
            return isinstance(data, (CompressedData, QuantizedCompressedData))
        return [isinstance(x, (CompressedData, QuantizedCompressedData)) for x in data]

    def _compress_one(self, data, name="[0]", **kwargs):
        raise NotImplementedError()

    def _decompress_one(self, data, name="[0]"):
        raise NotImplementedError()


# ---------------------------------------------------------------------------
# the payload
# ---------------------------------------------------------------------------
class SparseMask:
    """The positions of a device payload: ``index`` (flat, int32, ascending)
    and the 2-D ``shape``; what ``get_sparse_mask`` gives where scipy has no
    place."""

    __slots__ = ("index", "shape")

    def __init__(self, index, shape):
        self.index = index
        self.shape = tuple(int(d) for d in shape)


def _is_cuda(a) -> bool:
    return isinstance(a, torch.Tensor) and a.is_cuda


class SparseCompressedData(CompressedData):
    """One sparsified tensor: ``compressed_data`` (the kept values) and
    ``index`` (their flat positions, int32, strictly ascending) as two numpy
    arrays, two CPU tensors or two tensors on one GPU; ``sparse_rate``, the 2-D
    ``shape``, ``origin_shape`` and ``origin_type`` (the tensor's numpy dtype)."""

    def __init__(self, compressed_data, sparse_rate: float, index, shape, origin_shape, origin_type):
        super().__init__(compressed_data)
        self.sparse_rate = sparse_rate
        self.index = index
        self.shape = tuple(int(d) for d in shape)
        self.origin_shape = tuple(int(d) for d in origin_shape)
        self.origin_type = _np_dtype(origin_type)

    def _row_col(self):
        cols = max(self.shape[1], 1)
        if isinstance(self.index, torch.Tensor):
            idx = self.index.to(torch.int64)
            return torch.div(idx, cols, rounding_mode="floor"), idx % cols
        idx = self.index.astype(np.int64)
        return idx // cols, idx % cols

    @property
    def row(self):
        """The kept entries' rows in ``shape`` (int64), where the payload lives."""
        return self._row_col()[0]

    @property
    def col(self):
        return self._row_col()[1]

    @property
    def k(self) -> int:
        return int(self.index.numel() if isinstance(self.index, torch.Tensor) else self.index.size)

    @property
    def nbytes(self) -> int:
        """Index plus data: what travels."""
        return self.k * (4 + self.origin_type.itemsize)

    @property
    def is_device(self) -> bool:
        return _is_cuda(self.index)

    def to(self, device) -> "SparseCompressedData":
        """The same payload on ``device`` (a torch device): numpy arrays on the
        CPU, tensors on a GPU, through pinned memory."""
        device = torch.device(device)
        if device.type == "cpu":
            move = _host
        else:
            from .. import hostpipe as H

            move = lambda a: H.h2d(a, device)  # noqa: E731
        data = None if self.compressed_data is None else move(self.compressed_data)
        return SparseCompressedData(data, self.sparse_rate, move(self.index), self.shape, self.origin_shape,
                                    self.origin_type)

    def to_coo(self) -> SparseCOO:
        """A ``SparseCOO`` of ``origin_shape`` that shares ``index`` and the
        data: a top-k upload goes straight into ``SparsePlainAggregator``."""
        return SparseCOO(self.origin_shape, self.origin_type, self.index, self.compressed_data)

    def to_dense(self, name: str = "[0]"):
        """The dense tensor, decoded and validated where the payload lives."""
        if self.compressed_data is None:
            raise ValueError(f"sparse payload {name}: it carries no data (a MixedCompressor participant)")
        return _decode_one(self.to_coo(), name)

    def to_dense_numpy(self) -> np.ndarray:
        return _host(self.to_dense())

    def get_sparse_mask(self):
        """The kept positions: a scipy ``csr_matrix`` of bool in ``shape`` for
        a host payload, as the reference gives; a ``SparseMask`` for a device
        payload.  Every kept position is in it, whatever its value."""
        if self.is_device:
            return SparseMask(self.index, self.shape)
        from scipy import sparse as sp

        row, col = (_host(a) for a in self._row_col())
        return sp.csr_matrix((np.ones(row.size, dtype=bool), (row, col)), shape=self.shape)

    def __repr__(self):
        where = str(self.index.device) if isinstance(self.index, torch.Tensor) else "host"
        return f"SparseCompressedData(origin_shape={self.origin_shape}, dtype={self.origin_type}, k={self.k}, {where})"


def _mask_index(mask, shape2, device, name: str):
    """A mask's flat positions (int32, ascending) where the data lives:
    a tensor on ``device``, or a numpy array for ``device`` None."""
    if isinstance(mask, SparseMask):
        index, mshape = mask.index, mask.shape
    elif hasattr(mask, "tocoo"):
        m = mask.tocoo()
        on = np.asarray(m.data).astype(bool)
        flat = np.asarray(m.row)[on].astype(np.int64) * int(m.shape[1]) + np.asarray(m.col)[on].astype(np.int64)
        index, mshape = np.unique(flat).astype(np.int32), tuple(m.shape)
    else:
        raise TypeError(f"sparse entry {name}: sparse_mask is what get_sparse_mask() gives, not {type(mask)}")
    if tuple(mshape) != tuple(shape2):
        raise ValueError(f"sparse entry {name}: the mask is {tuple(mshape)}, the data {tuple(shape2)}")
    if device is None:
        return _host(index)
    if _is_cuda(index):
        return index.to(device)
    from .. import hostpipe as H

    return H.h2d(np.ascontiguousarray(_host(index)), device)


# ---------------------------------------------------------------------------
# the compressors
# ---------------------------------------------------------------------------
class SparseCompressor(Compressor):
    """The reference's ``SparseCompressor``; ``sparse_rate`` is the share of
    entries that are dropped."""

    def __init__(self, sparse_rate: float):
        assert 0 <= sparse_rate <= 1, f"sparse rate should between 0 and 1, but get {sparse_rate}"
        self.sparse_rate = sparse_rate

    def _decompress_one(self, data, name="[0]"):
        if not self.iscompressed(data):
            return data
        return data.to_dense(name)

    def _compress_one(self, data, name="[0]", sparse_mask=None):
        who = type(self).__name__
        tensor = isinstance(data, torch.Tensor)
        if not tensor:
            data = np.asarray(data)
        origin_shape = tuple(data.shape)
        if len(origin_shape) == 0:  # do not compress a scalar
            return data
        dt = _np_dtype(data.dtype)
        if dt not in _KEY:
            raise TypeError(f"{who}: entry {name} is {dt}; float32 or float64 data")
        n = _size(origin_shape)
        if n >= _MAX_N:
            raise ValueError(f"{who}: entry {name} has 2^31 elements or more: no int32 flat index")
        shape2 = (1, n) if len(origin_shape) == 1 else (origin_shape[0], _size(origin_shape[1:]))
        device = data.device if tensor and data.is_cuda else None
        if device is not None:
            flat = data.detach().contiguous().reshape(-1)
        else:
            flat = np.ascontiguousarray(data.detach().numpy() if tensor else data).reshape(-1)
        if sparse_mask is not None:
            index = _mask_index(sparse_mask, shape2, device, name)
            if device is not None:
                values = self._gather_device(flat, index)
            else:
                check_host_payload(index, n, name)
                values = flat[index]
        elif device is not None:
            index, values = self._select_device(flat, keep_count(self.sparse_rate, n))
        else:
            index = self._select_host(flat, keep_count(self.sparse_rate, n))
            values = flat[index]
        if tensor and device is None:  # a CPU tensor stays one
            index, values = torch.from_numpy(index), torch.from_numpy(values)
        return SparseCompressedData(values, self.sparse_rate, index, shape2, origin_shape, dt)

    @staticmethod
    def _gather_device(flat: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
        from .. import kernels as K

        index = index.contiguous()
        values = torch.empty(index.numel(), dtype=flat.dtype, device=flat.device)
        if index.numel():
            # an index outside the tensor is not used; it stays in the payload,
            # whose decompress validates it: nothing is read back here
            K.coo_gather(index, flat, values, K.coo_flag(flat.device))
        return values

    @staticmethod
    def _fill_device(keys: torch.Tensor, flat: torch.Tensor, k: int):
        """select + fill: (index, values) of the ``k`` largest ``keys``."""
        from .. import kernels as K
        from .compressor import _scratch_for

        index = torch.empty(k, dtype=torch.int32, device=flat.device)
        values = torch.empty(k, dtype=flat.dtype, device=flat.device)
        if k:
            scratch = _scratch_for(keys, K.topk_scratch_bytes(keys.numel(), keys.dtype))
            K.topk_select(keys, k, scratch)
            # keys do not change between the two calls (one stream), so the total is k and the flag
            # is not read; were it to differ, no entry beyond k would be stored
            K.topk_fill(keys, flat, k, scratch, index, values, K.coo_flag(flat.device))
        return index, values

    def _select_host(self, flat: np.ndarray, k: int) -> np.ndarray:
        raise NotImplementedError()

    def _select_device(self, flat: torch.Tensor, k: int):
        raise NotImplementedError()


class TopkSparse(SparseCompressor):
    """The reference's ``TopkSparse``; the module's docstring has the definition."""

    def _select_host(self, flat, k):
        return topk_index(flat, k)

    def _select_device(self, flat, k):
        return self._fill_device(flat, flat, k)


class RandomSparse(SparseCompressor):
    """The reference's ``RandomSparse`` with a keyed, reproducible draw; the
    module's docstring has the definition."""

    def __init__(self, sparse_rate: float, seed: int | None = None):
        super().__init__(sparse_rate)
        self.seed = secrets.randbits(64) if seed is None else int(seed) & _M64
        self.draws = 0  # tensors drawn so far: the next one uses seed + draws

    def _next_seed(self) -> int:
        s = (self.seed + self.draws) & _M64
        self.draws += 1
        return s

    def _select_host(self, flat, k):
        from .._lib import topk_random_keys_host

        return largest_keys_index(topk_random_keys_host(self._next_seed(), flat.size), k)

    def _select_device(self, flat, k):
        from .. import kernels as K

        seed = self._next_seed()
        if k == 0:
            return self._fill_device(flat, flat, 0)
        keys = torch.empty(flat.numel(), dtype=torch.float64, device=flat.device)
        return self._fill_device(K.topk_random_keys(seed, keys), flat, k)


# ---------------------------------------------------------------------------
# sparse + quantized
# ---------------------------------------------------------------------------
class MixedCompressedData(CompressedData):
    """``compressed_data``: the quantizer's codes of the kept values;
    ``compressed_participants``: the sparse and the quantized object, whose
    own data is ``None`` until ``decompress`` puts it back."""

    def __init__(self, compressed_data, compressed_participants: List):
        super().__init__(compressed_data)
        self.compressed_participants: list = compressed_participants

    def get_sparse_mask(self):
        return self.compressed_participants[0].get_sparse_mask()

    @property
    def nbytes(self) -> int:
        """Index plus codes: what travels besides a few scalars."""
        d = self.compressed_data
        codes = d.numel() * d.element_size() if isinstance(d, torch.Tensor) else int(d.nbytes)
        return 4 * self.compressed_participants[0].k + codes

    @property
    def is_device(self) -> bool:
        return _is_cuda(self.compressed_data)


class MixedCompressor(Compressor):
    """The reference's ``MixedCompressor``: exactly two compressors, a sparse
    one and a quantized one; given in the other order they are swapped with a
    warning, any other pairing raises ``RuntimeError``."""

    def __init__(self, *compressors):
        self.comressors = list(compressors)  # the reference's spelling
        assert len(self.comressors) == 2, "Only support 2 compressors (Sparse + Quantized)"
        if isinstance(self.comressors[0], QuantizedCompressor) and isinstance(self.comressors[1], SparseCompressor):
            self.comressors.reverse()
            logging.warning("In mixed compressors, sf will first use sparse compress and then use quantized compress.")
        if not (isinstance(self.comressors[0], SparseCompressor)
                and isinstance(self.comressors[1], QuantizedCompressor)):
            raise RuntimeError(f"Only support 2 compressors (Sparse + Quantized), got {type(self.comressors[0])} "
                               f"and {type(self.comressors[1])}")

    def _compress_one(self, data, name="[0]", sparse_mask=None):
        sparse_c, quant_c = self.comressors
        sparse_data = sparse_c._compress_one(data, name, sparse_mask=sparse_mask)
        if not isinstance(sparse_data, SparseCompressedData):  # a scalar passes through
            return sparse_data
        if sparse_data.k == 0:
            raise ValueError(f"mixed entry {name}: the sparse payload is empty (k == 0); a range of nothing cannot "
                             "be quantized")
        quant_data = quant_c._compress_one(sparse_data.compressed_data, name)
        codes = quant_data.compressed_data
        sparse_data.compressed_data = None
        quant_data.compressed_data = None
        return MixedCompressedData(codes, [sparse_data, quant_data])

    def _decompress_one(self, data, name="[0]"):
        if not isinstance(data, MixedCompressedData):
            return data
        sparse_c, quant_c = self.comressors
        sparse_data, quant_data = data.compressed_participants
        quant_data.compressed_data = data.compressed_data
        sparse_data.compressed_data = quant_c._decompress_one(quant_data, name)
        return sparse_c._decompress_one(sparse_data, name)


def get(name: str, params: Union[Dict, List, None]):
    """The reference's factory: a compressor by its name, ``params`` its
    keyword arguments; ``"mixed_compressor"`` takes a list of
    ``{"name": ..., "params": ...}``."""
    from .compressor import SCRSparse, STCSparse
    from .quantized import QuantizedFP, QuantizedKmeans, QuantizedLSTM, QuantizedZeroPoint

    simple = {"random_sparse": RandomSparse, "topk_sparse": TopkSparse, "stc_sparse": STCSparse,
              "scr_sparse": SCRSparse, "quantized_fp": QuantizedFP, "quantized_lstm": QuantizedLSTM,
              "quantized_zeropoint": QuantizedZeroPoint}
    if name in simple:
        return simple[name](**(params or {}))
    if name == "quantized_kmeans":
        if (params or {}).get("init") is None:
            raise ValueError("Compressor 'quantized_kmeans' is not built: scikit-learn's randomly initialised "
                             "k-means has no definition to pin; pass init='cbrt'")
        return QuantizedKmeans(**params)
    if name == "mixed_compressor":
        assert isinstance(params, list)
        parts = []
        for p in params:
            assert isinstance(p, dict) and "name" in p
            parts.append(get(p["name"], p.get("params")))
        return MixedCompressor(*parts)
    raise ValueError(f"Compressor '{name}' not exists.")
