"""HomoBinning: the reference's federated quantile binning
(``sfl/preprocessing/binning/homo_binning.py``, ``homo_binning_base.py``), the
step ``homo_booster.py:143-156`` runs before the first tree.  Its result is the
``bin_split_points`` that ``sfl_amd.ml.boost.FeatureHistogram`` takes.  The
parties' local work runs on host arrays in numpy and on CUDA tensors through
the ``sa_bin_*`` kernels, both forms with the same bits.

The definition
--------------
Party ``p`` holds ``x_p`` (``rows_p x F``, float32 or float64, contiguous, a
numpy array or a CUDA tensor, independently per party).

*Valid.*  A value of feature ``f`` is valid if it is not NaN and equals no entry
of ``abnormal_list``, compared in the data's dtype (``x == dtype(a)``).

*Range.*  Per party and feature: ``missing_f``, the number of NaN values;
``count_f``, the number of valid values; ``min_f`` and ``max_f`` over the valid
values as float64, a zero returned as ``+0.0``; ``+inf, -inf, 0`` for a feature
without a valid value.

*Rank.*  ``rank[f, j]`` is the number of valid ``x[r, f]`` with ``x[r, f] <
q[f, j]``, strictly, compared exactly (float32 data widened to float64), as
int64.  Infinities are ordinary values there.  The reference asks a
Greenwald-Khanna sketch, whose ranks are within ``2 error n`` of these; here
the local quantities are exact (``compress_thres`` and ``head_size``, the
sketch's parameters, are accepted and ignored).

*The loop.*  The reference's, in float64 on the host; the state is ``F x
bin_num`` nodes ``(value, min_value, max_value, error, fixed)``.

- The per-party ranges go to the server in the clear, as the reference's
  ``HDataFrame.min()`` / ``max()`` do; the global range of a feature is the
  min of the minima and the max of the maxima.  Everything else moves as sums
  through ``aggregator.sum(tables, axis=0)``: one table ``[rows, missing_0 ..
  missing_F-1, count_0 .. count_F-1]`` per party, then one ``F x bin_num``
  rank table per party and pass.  With ``aggregator=None`` the tables are
  summed plainly.
- ``total`` is the parties' rows together; ``error_rank = ceil(error *
  total)``; the query points start at ``np.linspace(min, max, bin_num +
  1)[1:]`` with the constructor's ``error``; ``aim_rank = floor(linspace(0, 1,
  bin_num + 1)[1:] * (total - missing_f))``.
- One pass: every party ranks the query points, the tables are summed.
- ``renew_query_points``: a fixed node stays; ``rank - aim_rank >
  error_rank`` moves left (``create_left_new``: ``value' = (value +
  min_value) / 2``, ``max_value' = value``), ``aim_rank - rank > error_rank``
  moves right (``create_right_new``, mirrored), anything else is fixed by
  rank.  A move with ``|value' - value| <= (max_value - min_value) * error *
  0.1``, on the node's own interval, fixes the node by width instead, where it
  is.  A new node takes the dataclass's default ``error = 1e-4``.
- After the first pass the loop renews, stops when every node is fixed
  (``check_converge``) and otherwise runs another pass, ``max_iter`` times at
  most: ``max_iter + 1`` passes when it does not converge.
- ``get_bin_result``: the nodes' values; unless ``allow_duplicate``, ``sorted(
  set(values))`` with values of magnitude below ``error`` replaced by ``0.0``
  and a value within ``error`` of its predecessor dropped, as the reference
  does it.  With ``allow_duplicate`` the values are returned sorted, which
  leaves an ascending list as it is (``FeatureHistogram`` asks for one).

A feature whose global range is not finite, or that has no valid value in any
party, raises ``ValueError``.

*Same bits.*  Counts and extrema do not depend on the order of the rows, so
host parties, device parties and any mix of them give the same split points
bit for bit.

The device form takes ``bin_num <= 255`` (``SA_BIN_MAX_Q``), at most 4
abnormal values (``SA_BIN_MAX_ABNORMAL``) and float32 or float64 data.  A
device party outside that takes the host form on a pinned copy of its data,
counted in ``last_report["host_fallback"]``.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

from ...device import PYUObject, reveal

MAX_Q, MAX_ABNORMAL = 255, 4  # _lib.SA_BIN_MAX_Q, _lib.SA_BIN_MAX_ABNORMAL
NODE_ERROR = 1e-4  # SplitPointNode.error's default: what a new node gets


def _is_cuda(t) -> bool:
    return bool(getattr(t, "is_cuda", False))


class HostWorker:
    """A party's local quantities in numpy: the definition, executable."""

    def __init__(self, x: np.ndarray, abnormal: Sequence[float]):
        self.x = x
        self.abnormal = [a for a in abnormal]
        self._sorted: dict = {}  # feature -> its valid values, ascending, float64

    def _valid(self, f: int) -> np.ndarray:
        col = self.x[:, f]
        ok = ~np.isnan(col)
        for a in self.abnormal:
            ok &= col != self.x.dtype.type(a)
        return ok

    def range(self):
        """``(min, max, count, missing)``, each over the ``F`` features."""
        nf = self.x.shape[1]
        mn, mx = np.full(nf, np.inf), np.full(nf, -np.inf)
        count, missing = np.zeros(nf, dtype=np.int64), np.zeros(nf, dtype=np.int64)
        for f in range(nf):
            v = self.x[self._valid(f), f].astype(np.float64)
            missing[f] = int(np.isnan(self.x[:, f]).sum())
            count[f] = v.size
            if v.size:
                mn[f], mx[f] = v.min() + 0.0, v.max() + 0.0  # -0.0 + 0.0 = +0.0
        return mn, mx, count, missing

    def ranks(self, cols: Sequence[int], q: np.ndarray) -> np.ndarray:
        """``rank[i, j]`` of the definition for feature ``cols[i]`` and query
        point ``q[i, j]`` (any order), int64."""
        out = np.empty(q.shape, dtype=np.int64)
        for i, f in enumerate(cols):
            if f not in self._sorted:
                self._sorted[f] = np.sort(self.x[self._valid(f), f].astype(np.float64))
            out[i] = np.searchsorted(self._sorted[f], q[i], side="left")
        return out


class DeviceWorker:
    """A party's local quantities through ``sa_bin_range`` / ``sa_bin_ranks``;
    one pinned read of the result table per call."""

    def __init__(self, x, abnormal: Sequence[float]):
        import torch

        self.x = x
        self.abnormal = [float(a) for a in abnormal]
        self._out = None
        self._torch = torch

    def range(self):
        from ... import hostpipe as H
        from ... import kernels as K

        out = self._torch.empty((self.x.shape[1], 4), dtype=self._torch.int64, device=self.x.device)
        w = H.d2h(K.bin_range(self.x, self.abnormal, out), pooled=False)
        return w[:, 0].copy().view(np.float64), w[:, 1].copy().view(np.float64), w[:, 2].copy(), w[:, 3].copy()

    def ranks(self, cols: Sequence[int], q: np.ndarray) -> np.ndarray:
        from ... import hostpipe as H
        from ... import kernels as K

        # the kernel takes ascending tables: sort and un-permute, as the reference's query_table does
        order = np.argsort(q, axis=1, kind="stable")
        table = np.full((self.x.shape[1], q.shape[1]), np.nan)  # a feature that is not binned counts nothing
        table[list(cols)] = np.take_along_axis(q, order, axis=1)
        if self._out is None or self._out.shape != table.shape:
            self._out = self._torch.empty(table.shape, dtype=self._torch.int64, device=self.x.device)
        K.bin_ranks(self.x, H.h2d(table, self.x.device), self.abnormal, self._out)
        got = H.d2h(self._out, pooled=False)[list(cols)]
        out = np.empty_like(got)
        np.put_along_axis(out, order, got, axis=1)
        return out


class HomoBinning:
    """``HomoBinning(bin_num=10, error=1e-4, max_iter=10, allow_duplicate=False,
    abnormal_list=None, bin_indexes=(), aggregator=None)``: see the module's
    docstring for the definition.  ``compress_thres`` and ``head_size`` are
    accepted and ignored: the local ranks are exact, there is no sketch."""

    def __init__(self, bin_num: int = 10, error: float = 1e-4, max_iter: int = 10, allow_duplicate: bool = False,
                 abnormal_list: Sequence[float] | None = None, bin_indexes: Sequence[int] = (), aggregator=None,
                 compress_thres: int = 10000, head_size: int = 10000):
        if int(bin_num) < 1:
            raise ValueError("HomoBinning: bin_num >= 1")
        self.bin_num = int(bin_num)
        self.error = float(error)
        self.max_iter = int(max_iter)
        self.allow_duplicate = bool(allow_duplicate)
        self.abnormal_list = list(abnormal_list) if abnormal_list is not None else []
        self.bin_indexes = [int(i) for i in bin_indexes]
        self.aggregator = aggregator
        self.last_report: dict = {"passes": 0, "fixed": 0.0, "error_rank": None, "host_fallback": 0, "ranks": None,
                                  "aim_ranks": None, "fixed_by_rank": None}

    # ---------------------------------------------------------------- parties
    def _worker(self, data):
        dtype = str(data.dtype).replace("torch.", "")
        if data.ndim != 2:
            raise ValueError("HomoBinning: a party's data is rows x F")
        if not (data.is_contiguous() if _is_cuda(data) else data.flags["C_CONTIGUOUS"]):
            raise ValueError("HomoBinning: a contiguous array")
        if _is_cuda(data):
            if self.bin_num <= MAX_Q and len(self.abnormal_list) <= MAX_ABNORMAL and dtype in ("float32", "float64"):
                return DeviceWorker(data, self.abnormal_list)
            from ... import hostpipe as H

            self.last_report["host_fallback"] += 1
            data = H.d2h(data, pooled=False)
        data = np.asarray(data)
        if data.dtype.kind != "f":
            data = data.astype(np.float64)
        return HostWorker(data, self.abnormal_list)

    def _sum(self, aggregator, owners, tables) -> np.ndarray:
        """The int64 sum of the parties' tables through ``aggregator.sum(...,
        axis=0)`` (any ``Aggregator``; a secure one decodes to float64, exact
        for counts below 2^53); plainly without one."""
        if aggregator is None:
            return np.sum(tables, axis=0).astype(np.int64)
        data = [t if o is None else PYUObject(o, t) for o, t in zip(owners, tables)]
        got = reveal(aggregator.sum(data, axis=0))
        if _is_cuda(got):
            from ... import hostpipe as H

            got = H.d2h(got, pooled=False)
        return np.rint(np.asarray(got, dtype=np.float64)).astype(np.int64).reshape(tables[0].shape)

    # -------------------------------------------------------------------- fit
    def fit_split_points(self, parts: Sequence, aggregator=None) -> list:
        """The split points of the binned features: a list of ascending float64
        arrays, what ``FeatureHistogram(bin_split_points)`` takes.  ``parts``:
        one ``rows_p x F`` array per party, ``PYUObject``s or plain arrays."""
        aggregator = self.aggregator if aggregator is None else aggregator
        if not parts:
            raise ValueError("HomoBinning: input data cannot be none")
        self.last_report.update(passes=0, host_fallback=0)
        owners = [p.device if isinstance(p, PYUObject) else None for p in parts]
        workers = [self._worker(p.data if isinstance(p, PYUObject) else p) for p in parts]
        nf = workers[0].x.shape[1]
        if any(w.x.shape[1] != nf for w in workers):
            raise ValueError("HomoBinning: every party holds the same features")
        cols = self.bin_indexes or list(range(nf))
        if any(c < 0 or c >= nf for c in cols):
            raise ValueError(f"HomoBinning: bin_indexes within 0..{nf - 1}")
        nb = self.bin_num

        ranges = [w.range() for w in workers]
        totals = self._sum(aggregator, owners, [np.concatenate([[w.x.shape[0]], r[3], r[2]]).astype(np.int64)
                                                for w, r in zip(workers, ranges)])
        total, missing, count = int(totals[0]), totals[1:1 + nf][cols], totals[1 + nf:][cols]
        lo = np.min([r[0] for r in ranges], axis=0)[cols]
        hi = np.max([r[1] for r in ranges], axis=0)[cols]
        for i, f in enumerate(cols):
            if count[i] == 0 or not (np.isfinite(lo[i]) and np.isfinite(hi[i])):
                raise ValueError(f"HomoBinning: feature {f} has no valid value or no finite range "
                                 f"(min {lo[i]}, max {hi[i]}, {count[i]} valid)")
        error_rank = float(np.ceil(self.error * total))
        st = {
            "value": np.stack([np.linspace(a, b, nb + 1)[1:] for a, b in zip(lo, hi)]),
            "lo": np.repeat(lo[:, None], nb, axis=1), "hi": np.repeat(hi[:, None], nb, axis=1),
            "error": np.full((len(cols), nb), self.error), "fixed": np.zeros((len(cols), nb), dtype=bool),
            "by_rank": np.zeros((len(cols), nb), dtype=bool),
        }
        aim = np.stack([np.floor(np.linspace(0, 1, nb + 1)[1:] * float(total - m)) for m in missing])

        def one_pass():
            self.last_report["passes"] += 1
            return self._sum(aggregator, owners, [w.ranks(cols, st["value"]) for w in workers])

        rank = one_pass()
        n_iter = 0
        while n_iter < self.max_iter:
            if self._renew(st, rank, aim, error_rank):
                break
            rank = one_pass()
            n_iter += 1
        self.last_report.update(fixed=float(st["fixed"].mean()), error_rank=error_rank, ranks=rank, aim_ranks=aim,
                                fixed_by_rank=st["by_rank"])
        return [self._bin_result(v) for v in st["value"]]

    @staticmethod
    def _renew(st: dict, rank: np.ndarray, aim: np.ndarray, allow: float) -> bool:
        """``renew_query_points`` over all nodes at once; True: all fixed."""
        v, lo, hi, err, fixed = st["value"], st["lo"], st["hi"], st["error"], st["fixed"]
        left = ~fixed & (rank - aim > allow)
        right = ~fixed & ~left & (aim - rank > allow)
        hit = ~fixed & ~left & ~right
        width = (hi - lo) * err * 0.1
        for move, bound in ((left, lo), (right, hi)):
            new = (v + bound) / 2
            stuck = move & (np.fabs(new - v) <= width)
            go = move & ~stuck
            fixed |= stuck
            (hi if bound is lo else lo)[go] = v[go]  # the new node's far bound is the old value
            v[go] = new[go]
            err[go] = NODE_ERROR
        fixed |= hit
        st["by_rank"] |= hit
        return bool(fixed.all())

    def _bin_result(self, values: np.ndarray) -> np.ndarray:
        """``get_bin_result`` for one feature."""
        if self.allow_duplicate:
            return np.sort(values)
        sp = sorted(set(float(v) for v in values))
        res = [sp[0] if np.fabs(sp[0]) > self.error else 0.0]
        last = sp[0]
        for v in sp[1:]:
            if np.fabs(v) < self.error:
                v = 0.0
            if np.abs(v - last) > self.error:
                res.append(v)
            last = v
        return np.array(res, dtype=np.float64)
