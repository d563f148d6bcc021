"""The plaintext aggregator for sparse (COO) uploads, mirroring
``sfl/security/aggregation/sparse_plain_aggregator.py:25-139``.

Over ``axis=0`` (the parties) a list of ``SparseCOO`` entries is never
decoded: a dense accumulator is zeroed, every party's non-zeros are added
into it in list order (``acc[i] = acc[i] + A(x) * A(w)``, multiply and add
rounded separately) and, for an average, divided once.  The server's work is
proportional to the non-zeros it receives, not to parties x elements.  Host
entries run numpy and give numpy arrays.  When entries of a layer are device
``SparseCOO``s the accumulator is a tensor on their device: one
``kernels.coo_axpy`` per party in list order, ``kernels.coo_finish`` for an
average, one read of the parties' flag records after the last party; the
result stays on the device and has the host path's bits.

Accumulator type ``A`` and divisor follow numpy, and the result equals
numpy's over the decoded arrays bit for bit (the sign of a zero apart: the
accumulator starts from ``+0.0``):

=========================  ====================================  ==================
call                       A                                     divisor
=========================  ====================================  ==================
``sum``                    the data's type T                     none
``average``, no weights    T                                     ``T(K)``
``average`` with weights   ``result_type(T, weights.dtype)``     ``sum(w)`` in A
=========================  ====================================  ==================

numpy reduces ``axis=0`` of the stacked parties left to right -- except for
tensors of at most one element, where the reduction runs along a contiguous
axis and numpy sums pairwise.  Those, every other ``axis``, dense entries and
integer entries are decoded and go through ``np.sum`` / ``np.average`` itself.
"""

from __future__ import annotations

from typing import List

import numpy as np
import torch

from ...device import PYU, DeviceObject
from ...utils import sparse as S
from .aggregator import Aggregator

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


def _to_host(x, name: str):
    c = S.as_coo(x, name)
    if c is not None:
        x = S._decode_one(c.to("cpu") if c.is_device else c, name)  # device entries: through pinned memory
    if isinstance(x, torch.Tensor):
        from ... import hostpipe as H

        return H.d2h(x, pooled=False) if x.is_cuda else x.detach().numpy()  # a dense device entry: a pinned copy
    return np.asarray(x)


class SparsePlainAggregator(Aggregator):
    """Plaintext sparse aggregator.

    The computation will be performed in (decoded) plaintext.

    Warnings:
        SparsePlainAggregator is for debugging purpose only.
        You should not use it in production.  Every party's update reaches
        the server in the clear: use it only where the updates are not
        private.

    Examples:
      >>> aggregator = SparsePlainAggregator(alice)
      >>> a = alice(lambda: sparse_encode([np.eye(3)]))()
      >>> b = bob(lambda: sparse_encode([np.eye(3)]))()
      >>> sum_a_b = aggregator.sum([a, b], axis=0)
      >>> reveal(sum_a_b)
    """

    accepts_sparse = True  # FLModel(sparse_transport="both") asks for it

    def __init__(self, device: PYU):
        assert isinstance(device, PYU), f"Accepts PYU only but got {type(device)}."
        self.device = device

    # ------------------------------------------------------------ one entry
    def _sparse_axis0(self, entries: List[S.SparseCOO], weights, average: bool, name: str):
        """K SparseCOOs of one shape and float type, added without decoding them."""
        T = entries[0].dtype
        K, shape, n = len(entries), entries[0].shape, entries[0].size
        if weights is not None:
            wgt = np.asarray(weights)
            if wgt.shape != (K,):
                raise ValueError("1D weights expected, one per party")
            A = np.result_type(T, wgt.dtype)
            scl = wgt.sum(axis=0, dtype=A)  # numpy's own sum of the weights (np.average)
            if np.any(scl == 0.0):
                raise ZeroDivisionError("Weights sum to zero, can't be normalized")
            ws = [float(w) for w in wgt]
        else:
            A, ws = T, [1.0] * K
            scl = T.type(K)
        for k, c in enumerate(entries):
            S._check_form(c, f"{name}, party {k}")
        dev = next((c.data.device for c in entries if c.is_device), None)
        if dev is not None and np.dtype(A) in _FLOATS:  # any other A (complex weights): numpy below
            return self._device_axis0(entries, ws, A, scl if average else None, dev, name).reshape(shape)
        acc = np.zeros(n, dtype=A)
        for k, (c, w) in enumerate(zip(entries, ws)):
            index, data = S._host(c.index), S._host(c.data)
            S.check_host_payload(index, n, f"{name}, party {k}")
            with np.errstate(invalid="ignore", over="ignore"):
                acc[index] = acc[index] + data.astype(A) * A.type(w)
        if average:
            with np.errstate(invalid="ignore", divide="ignore"):
                acc = acc / scl
        return acc.reshape(shape)

    @staticmethod
    def _device_axis0(entries: List[S.SparseCOO], ws: List[float], A, scl, dev, name: str) -> torch.Tensor:
        """The same sum on ``dev``: the accumulator is zeroed once, every
        party is one launch on one stream (a valid payload's indices are
        unique, so no two threads meet in an element), and the flag records
        of all parties are read once at the end."""
        from ... import kernels as K

        n = entries[0].size
        acc = torch.zeros(n, dtype=getattr(torch, np.dtype(A).name), device=dev)
        flags = torch.zeros((len(entries), 2), dtype=torch.int32, device=dev)
        flags[:, 1] = -1
        for k, (c, w) in enumerate(zip(entries, ws)):
            if not c.is_device or c.data.device != dev:
                c = c.to(dev)  # host entries among them: through pinned memory
            K.coo_axpy(c.index.contiguous(), c.data.contiguous(), w, acc, flags[k])
        if scl is not None:
            K.coo_finish(acc, float(scl))
        for k, (bits, _) in enumerate(S._read_words(flags)):
            err = S.flag_error(int(bits), n, f"{name}, party {k}")
            if err is not None:
                raise err
        return acc

    def _entry(self, xs: list, axis, weights, average: bool, name: str):
        """One layer's (or one single entry's) values of every party."""
        coos = [S.as_coo(x, name) for x in xs]
        if axis == 0 and all(c is not None for c in coos) and coos[0].dtype in _FLOATS and coos[0].size > 1 \
                and all(c.shape == coos[0].shape and c.dtype == coos[0].dtype for c in coos):
            return self._sparse_axis0(coos, weights, average, name)
        # every other case: numpy itself over the decoded arrays, as the reference does
        host = [_to_host(c if c is not None else x, f"{name}, party {k}") for k, (c, x) in enumerate(zip(coos, xs))]
        return np.average(host, axis=axis, weights=weights) if average else np.sum(host, axis=axis)

    def _run(self, data: List[DeviceObject], axis, weights, average: bool):
        assert data, "Data to aggregate should not be None or empty!"
        data = [d.to(self.device) for d in data]
        if isinstance(weights, (list, tuple)):
            weights = [w.to(self.device).data if isinstance(w, DeviceObject) else w for w in weights]

        def _agg(*parties):
            if isinstance(parties[0], (list, tuple)):
                return [self._entry(list(layer), axis, weights, average, f"layer {li}")
                        for li, layer in enumerate(zip(*parties))]
            return self._entry(list(parties), axis, weights, average, "entry")

        return self.device(_agg)(*data)

    # --------------------------------------------------------------- surface
    def sum(self, data: List[DeviceObject], axis=None) -> DeviceObject:
        """Sum of array elements over a given axis (``np.sum`` over the
        stacked parties; per layer for per-layer lists)."""
        return self._run(data, axis, None, False)

    def average(self, data: List[DeviceObject], axis=None, weights=None) -> DeviceObject:
        """Weighted average along the specified axis (``np.average``)."""
        return self._run(data, axis, weights, True)
