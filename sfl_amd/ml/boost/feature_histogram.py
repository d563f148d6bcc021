"""FeatureHistogram: the node histograms of the reference's homo_boost
(``sfl/ml/boost/homo_boost/tree_core/feature_histogram.py``), its only heavy
step, on host arrays in numpy and on CUDA tensors through the ``sa_hist_*``
kernels, both forms with the same bits.

The definition
--------------
One party holds ``x`` (``rows x F``, float32 or float64), per feature ``f`` an
ascending list of ``nb_f >= 0`` split points (ragged), ``grad`` and ``hess``
(``rows``, float32 or float64), ``node_of_row`` (``rows``, int32: the slot
``0 .. n_nodes - 1`` of the row's node in this batch, or ``-1`` for a row in
none) and ``valid_features`` (``{fid: bool}``, as in the reference).

*Codes.*  ``code[r, f]`` is the number of split points of feature ``f`` that
are ``<= x[r, f]``, compared in float64: ``0 .. nb_f``, and ``nb_f`` ("beyond")
for NaN.  The reference's bucket ``b`` (``x < split[b]``, cumulative from the
left) is exactly ``code <= b``, for repeated split points too.  Codes depend on
``x`` and the split points only: ``bind`` computes them once per data set.

*Fixed-point sums.*  Gradients are summed as integers, so the result does not
depend on the order of the sum: host and device give the same bits and a run
repeats itself (what XGBoost's GPU histogram does).  For ``v`` in (``grad``,
``hess``) separately, with ``max|v| = m 2^e``, ``m`` in ``[0.5, 1)`` (``math.
frexp``): ``k_v = 62 - e - ceil(log2(rows))`` (``62 - e`` for one row, ``0``
for ``max|v| == 0``) and ``q = int64(rint(ldexp(float64(v), k_v)))``.  No sum of
``q`` over any subset of the rows exceeds ``2^62``.  A NaN or an infinity in
``grad`` or ``hess`` raises ``ValueError``.

*Histogram.*  For slot ``s``, valid feature ``f`` and bucket ``b < nb_f``:
``G, H`` are the int64 sums of ``q_grad, q_hess`` over the rows with
``node_of_row == s`` and ``code <= b``, ``N`` their number, and the output
triple is ``(ldexp(float64(G), -k_grad), ldexp(float64(H), -k_hess),
float64(N))``.  Against the exact sums of the float values an entry is off by at
most ``N 2^-(k_v + 1)``: every row rounded once to the grid.

*use_missing.*  One more bucket, ``nb_f``: the node's totals over all its rows,
NaN and beyond-last included, minus bucket ``nb_f - 1`` (the totals themselves
for ``nb_f == 0``).  A documented refinement: this is what the reference's
``_bin_hist`` means to compute, but its ``t_data[1:].sum()`` slices rows
instead of columns and sums the feature values in.

*Output.*  One float64 array ``(n_nodes, F, Bmax [+ 1], 3)``, ``Bmax`` the
largest ``nb_f``; zeros beyond a feature's buckets, for a feature that is not
valid and for an empty node (the reference's ``_generate_empty_histogram``).  A
CUDA tensor for device inputs.  ``as_lists`` gives the reference's nested form,
per node a list over the features of ``(nb_f [+ 1], 3)`` arrays with ``[]`` for
a feature that is not valid: what ``Splitter.find_split`` consumes.

The device form takes lists of at most ``SA_HIST_MAX_BINS`` = 255 split points
a feature (uint8 codes).  A longer list takes the host form for device inputs
too (uint16 codes on the host), counted in ``last_report["host_fallback"]``.
The device form never reads back: codes another party made up that exceed
``Bmax`` are skipped there, where the host form raises.
"""
from __future__ import annotations

import math
from typing import Dict, Sequence

import numpy as np

MAX_BINS = 255  # _lib.SA_HIST_MAX_BINS


def scale_of(max_abs: float, rows: int) -> int:
    """``k_v`` of the definition for ``max|v| = max_abs`` over ``rows`` rows."""
    max_abs = float(max_abs)
    if not math.isfinite(max_abs):
        raise ValueError("FeatureHistogram: grad and hess must be finite (a NaN or an infinity among them)")
    if max_abs == 0.0:
        return 0
    return 62 - math.frexp(max_abs)[1] - (int(rows) - 1).bit_length()


def _is_cuda(t) -> bool:
    return bool(getattr(t, "is_cuda", False))


def _host(t) -> np.ndarray:
    if not _is_cuda(t):
        return np.asarray(t)
    from ... import hostpipe as H

    return H.d2h(t, pooled=False)


class FeatureHistogram:
    """``FeatureHistogram(bin_split_points, use_missing=False)``: see the
    module's docstring for the definition.

    ``bind(x)`` once per data set, ``set_gradients(grad, hess)`` once per tree,
    ``calculate_histogram(codes, node_of_row, n_nodes, valid_features)`` once
    per layer."""

    def __init__(self, bin_split_points: Sequence, use_missing: bool = False):
        self.splits = [np.asarray(s, dtype=np.float64).reshape(-1) for s in bin_split_points]
        for f, s in enumerate(self.splits):
            if np.isnan(s).any() or (s[1:] < s[:-1]).any():
                raise ValueError(f"FeatureHistogram: the split points of feature {f} must ascend (no NaN)")
        self.use_missing = bool(use_missing)
        self.n_features = len(self.splits)
        self.n_bins = np.array([len(s) for s in self.splits], dtype=np.int32)
        self.bmax = int(self.n_bins.max()) if self.n_features else 0
        self.offsets = np.zeros(self.n_features + 1, dtype=np.int32)
        np.cumsum(self.n_bins, out=self.offsets[1:])
        self.flat_splits = np.concatenate(self.splits) if self.n_features else np.zeros(0)
        self.last_report: dict = {"k_grad": None, "k_hess": None, "launches": 0, "slot_chunks": 0, "host_fallback": 0}
        self._grads = None  # (grad, hess, k_grad, k_hess), host arrays or device tensors
        self._dev: dict = {}  # device -> the tables and the scratch kept there

    @property
    def buckets(self) -> int:
        """Buckets per feature in the output array."""
        return self.bmax + (1 if self.use_missing else 0)

    @property
    def wide(self) -> bool:
        """More split points in some feature than the device form takes."""
        return self.bmax > MAX_BINS

    # ------------------------------------------------------------------ codes
    def bind(self, x):
        """The codes of ``x`` (``rows x F``, float32 or float64, contiguous):
        a numpy uint8 array for a host array, a uint8 tensor on its GPU for a
        CUDA tensor (numpy uint16 on the host for a ``wide`` list)."""
        cuda = _is_cuda(x)
        if x.ndim != 2 or x.shape[1] != self.n_features:
            raise ValueError(f"FeatureHistogram.bind: x is rows x {self.n_features}")
        if str(x.dtype).replace("torch.", "") not in ("float32", "float64"):
            raise TypeError(f"FeatureHistogram.bind: float32 or float64 data, not {x.dtype}")
        if not (x.is_contiguous() if cuda else x.flags["C_CONTIGUOUS"]):
            raise ValueError("FeatureHistogram.bind: a contiguous array")
        if cuda and not self.wide:
            import torch

            from ... import kernels as K

            t = self._tables(x.device)
            codes = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
            return K.hist_codes(x, t["splits"], t["offsets"], self.bmax, codes)
        if cuda:
            self.last_report["host_fallback"] += 1
        return self._codes_host(_host(x))

    def _codes_host(self, x: np.ndarray) -> np.ndarray:
        codes = np.empty(x.shape, dtype=np.uint16 if self.wide else np.uint8)
        for f, s in enumerate(self.splits):
            col = x[:, f].astype(np.float64)
            c = np.searchsorted(s, col, side="right")
            c[np.isnan(col)] = len(s)
            codes[:, f] = c
        return codes

    # -------------------------------------------------------------- gradients
    def set_gradients(self, grad, hess) -> None:
        """The gradients of a boosting round and their two scales: on the
        device one range pass each and one pinned read of the two maxima."""
        if _is_cuda(grad) != _is_cuda(hess) or grad.shape != hess.shape or grad.ndim != 1 or grad.dtype != hess.dtype:
            raise ValueError("FeatureHistogram.set_gradients: grad and hess are two vectors of one length, dtype and "
                             "place")
        rows = grad.shape[0]
        if _is_cuda(grad) and not self.wide:
            import torch

            from ... import hostpipe as H
            from ... import kernels as K

            if not grad.is_contiguous() or not hess.is_contiguous():
                raise ValueError("FeatureHistogram.set_gradients: contiguous vectors")
            out6 = torch.empty(6, dtype=grad.dtype, device=grad.device)
            scratch = torch.empty(K.quant_scratch_bytes(rows, grad.dtype), dtype=torch.uint8, device=grad.device)
            K.quant_range(grad, scratch, out6[:3])
            K.quant_range(hess, scratch, out6[3:])
            w = H.d2h(out6, pooled=False)
            mg, mh = w[2], w[5]
        else:
            grad, hess = np.ascontiguousarray(_host(grad)), np.ascontiguousarray(_host(hess))
            if grad.dtype not in (np.float32, np.float64):
                raise TypeError(f"FeatureHistogram.set_gradients: float32 or float64, not {grad.dtype}")
            with np.errstate(all="ignore"):
                mg = np.max(np.abs(grad)) if rows else 0.0
                mh = np.max(np.abs(hess)) if rows else 0.0
        kg, kh = scale_of(mg, rows), scale_of(mh, rows)
        self._grads = (grad, hess, kg, kh)
        self.last_report.update(k_grad=kg, k_hess=kh)

    # -------------------------------------------------------------- histogram
    def calculate_histogram(self, codes, node_of_row, n_nodes: int, valid_features: Dict[int, bool] | None = None,
                            as_lists: bool = False):
        """The float64 array ``(n_nodes, F, buckets, 3)`` of the batch, a CUDA
        tensor for CUDA codes; with ``as_lists`` the pair of it and its nested
        form.  ``valid_features`` ``None``: every feature is valid."""
        if self._grads is None:
            raise ValueError("FeatureHistogram.calculate_histogram: set_gradients first")
        n_nodes = int(n_nodes)
        valid = np.array([valid_features is None or bool(valid_features[f]) for f in range(self.n_features)], dtype=bool)
        if codes.ndim != 2 or codes.shape[1] != self.n_features or codes.shape[0] != self._grads[0].shape[0] \
                or node_of_row.shape != (codes.shape[0],):
            raise ValueError("FeatureHistogram.calculate_histogram: rows x F codes, and one slot and one gradient a row")
        if _is_cuda(codes):
            out = self._histogram_device(codes, node_of_row, n_nodes, valid)
        else:
            out = self._histogram_host(codes, _host(node_of_row), n_nodes, valid)
        return (out, self.as_lists(out, valid_features)) if as_lists else out

    def calculate_histogram_of_rows(self, codes, rows_of_nodes: Sequence, valid_features=None, as_lists: bool = False):
        """The reference's shape of call: ``rows_of_nodes[s]`` holds the row
        indices of node ``s`` (disjoint), instead of ``node_of_row``."""
        node = np.full(codes.shape[0], -1, dtype=np.int32)
        for s, idx in enumerate(rows_of_nodes):
            node[np.asarray(_host(idx), dtype=np.int64)] = s
        if _is_cuda(codes):
            from ... import hostpipe as H

            node = H.h2d(node, codes.device)
        return self.calculate_histogram(codes, node, len(rows_of_nodes), valid_features, as_lists)

    def as_lists(self, hist, valid_features: Dict[int, bool] | None = None) -> list:
        """The reference's nested form of a histogram array: per node a list
        over the features of ``(nb_f [+ 1], 3)`` arrays, ``[]`` for a feature
        that is not valid."""
        h = _host(hist)
        miss = 1 if self.use_missing else 0
        return [[h[s, f, :self.n_bins[f] + miss].copy() if valid_features is None or valid_features[f] else []
                 for f in range(self.n_features)] for s in range(h.shape[0])]

    def _histogram_host(self, codes: np.ndarray, node: np.ndarray, n_nodes: int, valid: np.ndarray) -> np.ndarray:
        grad, hess, kg, kh = self._grads
        grad, hess = _host(grad), _host(hess)
        ncodes = self.bmax + 1
        out = np.zeros((n_nodes, self.n_features, self.buckets, 3), dtype=np.float64)
        self.last_report.update(launches=0, slot_chunks=0)
        sel = (node >= 0) & (node < n_nodes)
        slot = node[sel].astype(np.int64)
        qg = np.rint(np.ldexp(grad[sel].astype(np.float64), kg)).astype(np.int64)
        qh = np.rint(np.ldexp(hess[sel].astype(np.float64), kh)).astype(np.int64)
        for f in np.flatnonzero(valid):
            nb = int(self.n_bins[f])
            c = codes[sel, f].astype(np.int64)
            if c.size and c.max() > nb:
                raise ValueError(f"FeatureHistogram: feature {f} has a code above its {nb} split points")
            at = slot * ncodes + c
            img = np.zeros((3, n_nodes * ncodes), dtype=np.int64)
            np.add.at(img[0], at, qg)
            np.add.at(img[1], at, qh)
            img[2] = np.bincount(at, minlength=n_nodes * ncodes)
            cum = np.cumsum(img.reshape(3, n_nodes, ncodes), axis=2)
            buckets = cum[:, :, :nb]
            if self.use_missing:
                last = cum[:, :, nb - 1] if nb else np.zeros((3, n_nodes), dtype=np.int64)
                buckets = np.concatenate([buckets, (cum[:, :, -1] - last)[:, :, None]], axis=2)
            for j, k in enumerate((kg, kh, 0)):
                out[:, f, :buckets.shape[2], j] = np.ldexp(buckets[j].astype(np.float64), -k)
        return out

    # ----------------------------------------------------------------- device
    def _tables(self, device) -> dict:
        """The split points, their offsets and the scratch on ``device``."""
        t = self._dev.get(device)
        if t is None:
            from ... import hostpipe as H

            t = {"splits": H.h2d(self.flat_splits, device), "offsets": H.h2d(self.offsets, device), "n_bins": {},
                 "scratch": None}
            self._dev[device] = t
        return t

    def _histogram_device(self, codes, node_of_row, n_nodes: int, valid: np.ndarray):
        import torch

        from ... import hostpipe as H
        from ... import kernels as K

        grad, hess, kg, kh = self._grads
        if self.wide or not _is_cuda(grad) or not _is_cuda(node_of_row):
            raise ValueError("FeatureHistogram.calculate_histogram: device codes go with device gradients and slots "
                             f"and lists of at most {MAX_BINS} split points")
        dev = codes.device
        out = torch.empty((n_nodes, self.n_features, self.buckets, 3), dtype=torch.float64, device=dev)
        self.last_report.update(launches=0, slot_chunks=0)
        if out.numel() == 0:
            return out
        t = self._tables(dev)
        key = valid.tobytes()
        if key not in t["n_bins"]:  # one small upload per set of valid features
            t["n_bins"][key] = H.h2d(np.where(valid, self.n_bins, -1).astype(np.int32), dev)
        need = K.hist_scratch_bytes(n_nodes, self.n_features, self.bmax)
        if t["scratch"] is None or t["scratch"].numel() < need:
            t["scratch"] = torch.empty(need, dtype=torch.uint8, device=dev)
        K.hist_build(codes, self.bmax, node_of_row, n_nodes, grad, hess, kg, kh, t["scratch"])
        K.hist_finish(t["scratch"], n_nodes, self.n_features, self.bmax, t["n_bins"][key], kg, kh, self.use_missing, out)
        chunks = K.hist_geometry(self.bmax, n_nodes, self.n_features)[2] if codes.shape[0] else 0
        self.last_report.update(launches=2 + chunks, slot_chunks=chunks)
        return out
